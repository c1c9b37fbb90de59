"""Sliding-window (banded causal) attention, stated in NumPy: with `causal=True` and a window W >= 1, query i (absolute
position i + start_pos) sees key j iff

    max(0, i + start_pos - W + 1) <= j <= i + start_pos

-- the last W keys up to its own (Mistral, the local layers of Gemma 2 / 3, Phi-3).  A key outside the band has probability
exactly 0 and receives exactly 0 gradient from that query; a key no query sees gets dk = dv = 0.  `window=None` is plain
causal attention, and so is any W >= start_pos + Lq.  A window needs `causal=True` and Lk >= start_pos + Lq (every query
sees at least its own key); otherwise ValueError.

q, k, v: (B, L, H, hd), as many key/value heads as query heads.  This is what `fused.attention(..., window=W)` evaluates on
the `cpu` device and what the kernels of csrc/attention_band.hip (include/pdn_bandattn.h) are held to; those take no mask
operand: the key range of a query tile is a function of its index."""
import math

import numpy as np


def check(window, causal, Lq, Lk, start_pos):
    """`window` as an int (None passes through); ValueError for one that is no positive integer, without `causal`, or
    with fewer keys than start_pos + Lq."""
    if window is None:
        return None
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"attention: window must be a positive integer or None, got {window!r}")
    if not causal:
        raise ValueError("attention: window needs causal=True")
    if Lk < start_pos + Lq:
        raise ValueError(f"attention: window needs Lk >= start_pos + Lq (every query sees its own key), got Lk = {Lk}, "
                         f"start_pos = {start_pos}, Lq = {Lq}")
    return int(window)


def band_mask(Lq, Lk, start_pos, W, dtype):
    """(Lq, Lk) additive: 0 inside the band, -inf where key > query + start_pos or key < query + start_pos - W + 1."""
    keys, pos = np.arange(Lk)[None, :], np.arange(Lq)[:, None] + start_pos
    return np.where((keys > pos) | (keys < pos - W + 1), -np.inf, 0.0).astype(dtype)


def forward(q, k, v, causal=True, start_pos=0, window=None):
    """(o (B, Lq, H, hd), lse (B, H, Lq), p (B, H, Lq, Lk))"""
    B, Lq, H, hd = q.shape
    Lk = k.shape[1]
    W = check(window, causal, Lq, Lk, start_pos)
    s = np.matmul(q.transpose(0, 2, 1, 3), k.transpose(0, 2, 3, 1)) / np.asarray(math.sqrt(hd), q.dtype)
    if causal:
        s = s + band_mask(Lq, Lk, start_pos, Lk if W is None else W, q.dtype)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    z = e.sum(-1, keepdims=True)
    p = e / z
    o = np.ascontiguousarray(np.matmul(p, v.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3))
    return o, (m + np.log(z))[..., 0], p


def backward(q, k, v, p, do):
    """(dq, dk, dv) from the probabilities `p` of `forward`: p is exactly 0 outside the band, and so are dS and every
    contribution to dk / dv from there."""
    hd = q.shape[3]
    doT = do.transpose(0, 2, 1, 3)
    dv = np.matmul(p.swapaxes(-1, -2), doT).transpose(0, 2, 1, 3)
    dp = np.matmul(doT, v.transpose(0, 2, 3, 1))
    ds = (dp - (dp * p).sum(-1, keepdims=True)) * p / np.asarray(math.sqrt(hd), q.dtype)
    dq = np.matmul(ds, k.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
    dk = np.matmul(ds.swapaxes(-1, -2), q.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(dq), np.ascontiguousarray(dk), np.ascontiguousarray(dv)
