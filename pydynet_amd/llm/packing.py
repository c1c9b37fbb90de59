"""Packing documents of different lengths into fixed-length training rows (pure NumPy).

    input_ids, target_ids, segment_ids = pack_sequences(documents, seq_len)
    model.finetune_step(input_ids, target_ids.reshape(-1), optimizer, ignore_index=-100, segment_ids=segment_ids)

One document per row, padded to the sequence length, spends every GEMM and the whole attention triangle on padding; several
documents in one row under plain causal attention let each document read the ones in front of it.  `segment_ids` is what
keeps the documents of a packed row apart (core/fused/segments.py): equal ids are one document, and the padding at the end of
a row is one more segment of its own.

Positions are not reset at a document's start: a rotary score depends on the distance between query and key only.
"""
import numpy as np


def pack_sequences(sequences, seq_len, pad_id=0, ignore_index=-100):
    """First-fit packing, in the given order, of token sequences into rows of `seq_len` positions.

    Returns (input_ids, target_ids, segment_ids), each (rows, seq_len): int64, int64 and int32.  A document longer than
    `seq_len` is split into pieces of `seq_len` tokens (the last one shorter), each piece a document of its own.  Every
    piece goes into the first row that still has room for it; a new row is opened when none has.  Targets are the next
    token INSIDE the piece: the last token of every piece and all padding carry `ignore_index`, so no target crosses a
    document boundary.  Segment ids count the pieces of a row from 0; the padding at the end of a row takes the next id.
    Empty sequences are dropped."""
    seq_len = int(seq_len)
    if seq_len < 1:
        raise ValueError("pack_sequences: seq_len must be at least 1")
    pieces = []
    for doc in sequences:
        doc = np.asarray(doc).reshape(-1)
        if doc.size and doc.dtype.kind not in "iu":
            raise ValueError("pack_sequences: token ids must be integers")
        for lo in range(0, doc.size, seq_len):
            pieces.append(doc[lo:lo + seq_len].astype(np.int64))
    rows, used = [], []                                  # rows: lists of pieces; used: tokens taken in each row
    for piece in pieces:
        for r, n in enumerate(used):
            if n + piece.size <= seq_len:
                rows[r].append(piece)
                used[r] += piece.size
                break
        else:
            rows.append([piece])
            used.append(piece.size)
    R = len(rows)
    input_ids = np.full((R, seq_len), pad_id, np.int64)
    target_ids = np.full((R, seq_len), ignore_index, np.int64)
    segment_ids = np.zeros((R, seq_len), np.int32)
    for r, row in enumerate(rows):
        at = 0
        for s, piece in enumerate(row):
            n = piece.size
            input_ids[r, at:at + n] = piece
            target_ids[r, at:at + n - 1] = piece[1:]
            segment_ids[r, at:at + n] = s
            at += n
        segment_ids[r, at:] = len(row)
    return input_ids, target_ids, segment_ids


def unpack_sequences(input_ids, segment_ids):
    """The pieces of packed rows, row by row and in order of position, the padding segment of each row included (the
    inverse of `pack_sequences` up to the order of the rows' pieces and the trailing padding pieces)."""
    out = []
    for ids, seg in zip(np.asarray(input_ids), np.asarray(segment_ids)):
        cuts = np.flatnonzero(np.diff(seg)) + 1
        out.append(np.split(ids, cuts))
    return out
