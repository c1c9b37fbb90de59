"""Document-masked ("packed", "varlen") causal attention, stated once in float64 array arithmetic.

This module is the contract of the segmented kernels (the SEG forms of csrc/attention.hip and the bounds kernel of
csrc/segments.hip; entries of include/pdn_segattn.h, prefix pdns_), as masked_loss.py is for the masked cross entropy; the
emulator part and the tests compare against it.  The reference's attention (llm/llama/model.py:112-121) masks by causality
alone: this is an extension.

    seg        (B, L) integers, non-decreasing along each row; equal ids are one document.  Padding at the end of a row
               is one more segment of its own.
    start[b,i] the smallest j with seg[b,j] == seg[b,i]
    end[b,i]   one past the largest such j
    query i sees key j  iff  start[b,i] <= j <= i

A key outside that range has probability exactly 0 and receives exactly 0 gradient from that query, so the documents of a
row neither read nor change each other: packing several of them into one row computes what they compute alone.

Positions are not reset at a document's start.  A rotary score depends on the distance between query and key only, so
a document that begins at position 137 scores as it would at position 0, up to rounding.

A row that decreases somewhere is an error (`check`; the device raises its error flag and falls back to plain causal bounds,
start 0 and end L).
"""
import numpy as np


def check(seg):
    """(B, L) integer ids as an int64 array; ValueError for another shape or dtype, or a row that decreases."""
    s = np.asarray(seg)
    if s.ndim != 2 or s.dtype.kind not in "iu":
        raise ValueError(f"segment_ids must be a (B, L) integer array, got shape {s.shape} and dtype {s.dtype}")
    s = s.astype(np.int64)
    if s.shape[1] > 1 and (np.diff(s, axis=1) < 0).any():
        b = int(np.argwhere(np.diff(s, axis=1) < 0)[0][0])
        raise ValueError(f"segment_ids must be non-decreasing along each row; row {b} decreases")
    return s


def decreasing_rows(seg):
    """(B,) bool: the rows that decrease somewhere."""
    s = np.asarray(seg).astype(np.int64)
    return (np.diff(s, axis=1) < 0).any(axis=1) if s.shape[1] > 1 else np.zeros(s.shape[0], bool)


def bounds(seg):
    """(start, end), both (B, L) int64.  A row that decreases gets the bounds of plain causal attention, 0 and L (what the
    device does beside raising its flag)."""
    s = np.asarray(seg).astype(np.int64)
    B, L = s.shape
    idx = np.broadcast_to(np.arange(L), (B, L))
    opens = np.ones((B, L), bool)
    opens[:, 1:] = s[:, 1:] != s[:, :-1]
    closes = np.ones((B, L), bool)
    closes[:, :-1] = s[:, :-1] != s[:, 1:]
    start = np.maximum.accumulate(np.where(opens, idx, 0), axis=1)
    end = np.minimum.accumulate(np.where(closes, idx + 1, L)[:, ::-1], axis=1)[:, ::-1]
    bad = decreasing_rows(s)
    start[bad], end[bad] = 0, L
    return start, np.ascontiguousarray(end)


def visible(start):
    """(B, L, L) bool, [b, i, j] = query i sees key j."""
    start = np.asarray(start)
    L = start.shape[1]
    j = np.arange(L)
    return (j[None, None, :] >= start[:, :, None]) & (j[None, None, :] <= j[None, :, None])


def additive_mask(start, dtype=np.float64):
    """(B, 1, L, L): 0 where the query sees the key, -inf elsewhere (the causal part included)."""
    return np.where(visible(start), 0.0, -np.inf).astype(dtype)[:, None]


def block_mask(start, dtype=np.float64):
    """(B, 1, L, L): -inf for the keys in front of the query's document, 0 elsewhere -- what is ADDED beside a causal
    mask that is applied on its own."""
    start = np.asarray(start)
    j = np.arange(start.shape[1])
    return np.where(j[None, None, :] < start[:, :, None], -np.inf, 0.0).astype(dtype)[:, None]


def rotate(x, cos, sin, sign=1.0):
    """RoPE on (B, L, H, hd): interleaved pairs (x[2i], x[2i+1]) by the angle of the position; sign -1 rotates back."""
    x = np.asarray(x, np.float64)
    c = np.asarray(cos, np.float64)[None, :, None, :]
    s = sign * np.asarray(sin, np.float64)[None, :, None, :]
    out = np.empty_like(x)
    out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return out


def attention_forward(q, k, v, start):
    """(o, lse, p) in float64.  q, k, v: (B, L, H, hd) as the kernels meet them (rotated, if at all); o: (B, L, H, hd),
    lse: (B, H, L), p: (B, H, L, L) with exact zeros outside the visible range."""
    q, k, v = (np.asarray(a, np.float64).transpose(0, 2, 1, 3) for a in (q, k, v))
    hd = q.shape[-1]
    s = np.matmul(q, k.swapaxes(-1, -2)) / np.sqrt(float(hd)) + additive_mask(start)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    z = e.sum(-1, keepdims=True)
    p = e / z
    return np.matmul(p, v).transpose(0, 2, 1, 3), (m + np.log(z))[..., 0], p


def attention_backward(q, k, v, d_o, start):
    """(dq, dk, dv) in float64, each (B, L, H, hd), with respect to q, k, v as given."""
    o, _, p = attention_forward(q, k, v, start)
    qt, kt, vt, ot, gt = (np.asarray(a, np.float64).transpose(0, 2, 1, 3) for a in (q, k, v, o, d_o))
    hd = qt.shape[-1]
    delta = (gt * ot).sum(-1, keepdims=True)
    dp = np.matmul(gt, vt.swapaxes(-1, -2))
    ds = p * (dp - delta) / np.sqrt(float(hd))
    dv = np.matmul(p.swapaxes(-1, -2), gt)
    dq = np.matmul(ds, kt)
    dk = np.matmul(ds.swapaxes(-1, -2), qt)
    return tuple(a.transpose(0, 2, 1, 3) for a in (dq, dk, dv))
