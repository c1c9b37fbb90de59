"""llm/packing.py: first-fit packing of documents into training rows (pure NumPy, no device)."""
import numpy as np
import pytest

from pydynet_amd.core.fused import segments as S
from pydynet_amd.llm.packing import pack_sequences, unpack_sequences

IGNORE = -100


def _docs(seed, n, lo, hi, vocab=1000):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, vocab, int(k)) for k in rng.integers(lo, hi + 1, n)]


def test_shapes_dtypes_and_segments():
    docs = _docs(1, 40, 3, 60)
    ids, tgt, seg = pack_sequences(docs, 64, pad_id=0, ignore_index=IGNORE)
    assert ids.shape == tgt.shape == seg.shape and ids.shape[1] == 64
    assert ids.dtype == np.int64 and tgt.dtype == np.int64 and seg.dtype == np.int32
    assert (np.diff(seg, axis=1) >= 0).all() and (seg[:, 0] == 0).all()          # the contract of segment_ids
    assert np.array_equal(S.check(seg), seg)
    assert ids.shape[0] < len(docs)                                              # it does pack
    assert sum(d.size for d in docs) <= ids.size


def test_first_fit_placement_in_the_given_order():
    # rows of 10: 6 opens row 0; 5 does not fit, opens row 1; 4 fits row 0 (full); 5 fits row 1 (full); 3 opens row 2; 1 -> row 2
    docs = [np.full(n, v) for v, n in enumerate((6, 5, 4, 5, 3, 1), start=1)]
    ids, tgt, seg = pack_sequences(docs, 10, pad_id=0)
    assert ids.tolist() == [[1] * 6 + [3] * 4, [2] * 5 + [4] * 5, [5] * 3 + [6] + [0] * 6]
    assert seg.tolist() == [[0] * 6 + [1] * 4, [0] * 5 + [1] * 5, [0] * 3 + [1] + [2] * 6]
    # a full row has no padding segment; padding is a segment of its own and carries no target
    assert (tgt[2, 4:] == IGNORE).all()


def test_long_documents_are_split():
    doc = np.arange(1, 26)
    ids, tgt, seg = pack_sequences([doc, np.array([77, 78])], 10)
    assert ids.shape == (3, 10)
    assert ids[0].tolist() == list(range(1, 11)) and ids[1].tolist() == list(range(11, 21))
    assert ids[2].tolist() == [21, 22, 23, 24, 25, 77, 78, 0, 0, 0]
    assert seg[2].tolist() == [0] * 5 + [1] * 2 + [2] * 3
    # the pieces are documents of their own: the last token of a piece has no target
    assert tgt[0].tolist() == list(range(2, 11)) + [IGNORE]
    assert tgt[2].tolist() == [22, 23, 24, 25, IGNORE, 78, IGNORE, IGNORE, IGNORE, IGNORE]


def test_no_target_crosses_a_document_boundary():
    docs = _docs(2, 60, 1, 50)
    ids, tgt, seg = pack_sequences(docs, 48, pad_id=0, ignore_index=IGNORE)
    start, end = S.bounds(seg)
    pos = np.broadcast_to(np.arange(48), ids.shape)
    last = pos == end - 1
    assert (tgt[last] == IGNORE).all()                                           # the last token of every segment, padding included
    inner = ~last
    nxt = np.roll(ids, -1, axis=1)
    padding = seg == seg.max(axis=1, keepdims=True)
    padding &= (ids == 0)
    real = inner & ~padding
    assert np.array_equal(tgt[real], nxt[real])                                  # the next token of the same document
    assert (tgt[padding] == IGNORE).all()
    n_valid = sum(d.size - -(-d.size // 48) for d in docs)                       # every piece loses its last token's target
    assert int((tgt != IGNORE).sum()) == n_valid


def test_decoding_the_rows_by_segment_gives_back_the_documents():
    docs = _docs(3, 50, 1, 90)
    ids, tgt, seg = pack_sequences(docs, 64, pad_id=0)
    pieces = []
    for d in docs:
        pieces += [d[lo:lo + 64] for lo in range(0, d.size, 64)]
    got = []
    for row in unpack_sequences(ids, seg):
        # (tokens are >= 1 and pad_id is 0: an all-zero last piece is the row's padding segment)
        got += row[:-1] if (row[-1] == 0).all() else row
    # first-fit keeps the order inside a row, not across rows: compare as multisets of token tuples
    assert sorted(tuple(p.tolist()) for p in got) == sorted(tuple(p.tolist()) for p in pieces)
    assert sum(p.size for p in got) == sum(d.size for d in docs)


def test_arguments():
    with pytest.raises(ValueError):
        pack_sequences([[1, 2]], 0)
    with pytest.raises(ValueError):
        pack_sequences([np.array([0.5, 1.5])], 8)
    ids, tgt, seg = pack_sequences([[], [4, 5, 6]], 4, pad_id=9, ignore_index=-1)
    assert ids.tolist() == [[4, 5, 6, 9]] and tgt.tolist() == [[5, 6, -1, -1]] and seg.tolist() == [[0, 0, 0, 1]]
    ids, tgt, seg = pack_sequences([], 4)
    assert ids.shape == (0, 4)
