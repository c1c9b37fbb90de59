"""Grouped-query attention, stated in NumPy: H query heads share Hkv key/value heads, query head h reads key/value
head h // G with G = H // Hkv (the `repeat_interleave` convention of the Llama family).

q: (B, Lq, H, hd); k, v: (B, Lk, Hkv, hd).  The output, dq and the saved lse are what multi-head attention gives on K / V
repeated G times along the head axis; dk[:, :, j] and dv[:, :, j] are the sums of the expanded gradients over heads
j * G .. j * G + G - 1.  `causal`, `start_pos` and the additive `mask` (broadcastable to (B, H, Lq, Lk), its head axis the
QUERY head) mean what they mean in `fused.attention`.  This is what `fused.attention` evaluates on the `cpu` device and
what the kernels of csrc/attention_gqa.hip (include/pdn_gqattn.h) are held to; those never form the repeated K / V."""
import math

import numpy as np


def group_size(H, Hkv):
    """G = H // Hkv; ValueError unless Hkv divides H."""
    if Hkv < 1 or H % Hkv:
        raise ValueError(f"attention: {H} query heads cannot share {Hkv} key/value heads (n_kv_heads must divide n_heads)")
    return H // Hkv


def expand(x, G):
    """(B, L, Hkv, hd) -> (B, L, Hkv * G, hd): head j repeated G times in place (heads j * G .. j * G + G - 1)."""
    return x if G == 1 else np.repeat(x, G, axis=2)


def reduce_groups(dx, G):
    """The transpose of `expand`: (B, L, Hkv * G, hd) -> (B, L, Hkv, hd), summed over each group."""
    if G == 1:
        return dx
    B, L, H, hd = dx.shape
    return dx.reshape(B, L, H // G, G, hd).sum(3)


def causal_mask(Lq, Lk, start_pos, dtype):
    """(Lq, Lk) additive: -inf where key > query + start_pos."""
    keys, queries = np.arange(Lk)[None, :], np.arange(Lq)[:, None]
    return np.where(keys > queries + start_pos, -np.inf, 0.0).astype(dtype)


def forward(q, k, v, causal=False, start_pos=0, mask=None):
    """(o (B, Lq, H, hd), lse (B, H, Lq), p (B, H, Lq, Lk))"""
    B, Lq, H, hd = q.shape
    G = group_size(H, k.shape[2])
    ke, ve = expand(k, G), expand(v, G)
    s = np.matmul(q.transpose(0, 2, 1, 3), ke.transpose(0, 2, 3, 1)) / np.asarray(math.sqrt(hd), q.dtype)
    if causal:
        s = s + causal_mask(Lq, k.shape[1], start_pos, q.dtype)
    if mask is not None:
        s = s + np.asarray(mask, q.dtype)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    z = e.sum(-1, keepdims=True)
    p = e / z
    o = np.ascontiguousarray(np.matmul(p, ve.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3))
    return o, (m + np.log(z))[..., 0], p


def backward(q, k, v, p, do):
    """(dq, dk, dv) from the probabilities `p` of `forward`: dk / dv summed over each group."""
    hd = q.shape[3]
    G = group_size(q.shape[2], k.shape[2])
    ke, ve = expand(k, G), expand(v, G)
    doT = do.transpose(0, 2, 1, 3)
    dv = np.matmul(p.swapaxes(-1, -2), doT).transpose(0, 2, 1, 3)
    dp = np.matmul(doT, ve.transpose(0, 2, 3, 1))
    ds = (dp - (dp * p).sum(-1, keepdims=True)) * p / np.asarray(math.sqrt(hd), q.dtype)
    dq = np.matmul(ds, ke.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
    dk = np.matmul(ds.swapaxes(-1, -2), q.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(dq), np.ascontiguousarray(reduce_groups(dk, G)), np.ascontiguousarray(reduce_groups(dv, G))
