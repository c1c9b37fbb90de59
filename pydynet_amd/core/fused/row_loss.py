"""Cross entropy with reduction='none', stated once in float64 array arithmetic.

This module is the contract of the row kernels in csrc/row_loss.hip (entries of include/pdn_rowloss.h, prefix pdnr_), as
masked_loss.py is for the masked kernels; the emulator part and the tests compare against it.  The reference's cross
entropy (nn/functional.py:364-381) reduces to a scalar: this is an extension.

    valid_n = ignore_index is None or t_n != ignore_index
    row_n   = logsumexp(z_n) - z_n[t_n]  for valid rows, 0 for ignored ones         the node's value, shape (rows,)
    u       = upstream gradient, shape (rows,): one number per row
    dz_n    = (softmax(z_n) - onehot(t_n)) * u_n  for valid rows, 0.0 exactly for ignored ones WHATEVER u_n holds (NaN too)
    lm_head : dx = dz W^T,  dW = x^T dz,  dbias = sum_n dz_n;  dx rows of ignored tokens are exactly 0

No count and no factor: a caller that wants a mean divides by what it wants to divide by (tokens, documents, weights).
A target that is valid and not inside [0, V) is an error (the device raises its error flag).

The lm_head node keeps its products: they form dz' = (softmax - onehot) * s from the saved logits with ONE device scalar s,
so the weight gradient is written  dW = (diag(u / s) x)^T dz'  with  s = max |u_n| over valid rows.  The normaliser is
needed: the split-fp16 product cuts x into fp16 planes with one exponent per feature column, and rows scaled by
u ~ 1 / rows would fall into fp16's subnormal range.  s == 0 (`abs_max` returns 1 / s = 0) gives dW = 0.
"""
import numpy as np


def valid_rows(targets, ignore_index):
    t = np.asarray(targets).reshape(-1)
    return np.ones(t.shape, bool) if ignore_index is None else t != int(ignore_index)


def check_targets(targets, ignore_index, V):
    """IndexError for a valid target that is not a class."""
    t = np.asarray(targets).reshape(-1)
    bad = valid_rows(t, ignore_index) & ((t < 0) | (t >= V))
    if bad.any():
        raise IndexError(f"cross entropy target {int(t[bad][0])} is neither ignore_index nor inside [0, {V})")


def _lse(z):
    m = z.max(-1, keepdims=True)
    return np.log(np.exp(z - m).sum(-1, keepdims=True)) + m


def rows(logits, targets, ignore_index=None):
    """the node's value: (rows,) float64, 0 at ignored rows"""
    z = np.asarray(logits, np.float64)
    t = np.asarray(targets).reshape(-1)
    check_targets(t, ignore_index, z.shape[1])
    valid = valid_rows(t, ignore_index)
    return np.where(valid, _lse(z)[:, 0] - z[np.arange(len(t)), np.where(valid, t, 0)], 0.0)


def dlogits(logits, targets, upstream, ignore_index=None):
    """(rows, V) float64 gradient of sum_n u_n row_n; ignored rows are 0 by a select, not by a product"""
    z = np.asarray(logits, np.float64)
    t = np.asarray(targets).reshape(-1)
    check_targets(t, ignore_index, z.shape[1])
    valid = valid_rows(t, ignore_index)
    u = np.where(valid, np.asarray(upstream, np.float64).reshape(-1), 0.0)
    d = np.exp(z - _lse(z))
    d[np.arange(len(t)), np.where(valid, t, 0)] -= 1.0
    d *= u[:, None]
    d[~valid] = 0.0
    return d


def abs_max(upstream, valid):
    """(s, 1 / s) with s the largest |u_n| over valid rows; (0, 0) when that is 0 or no row is valid"""
    u = np.abs(np.asarray(upstream, np.float64).reshape(-1)[np.asarray(valid, bool)])
    s = float(u.max()) if u.size else 0.0
    return s, (1.0 / s if s > 0.0 else 0.0)


def scale_rows(a, upstream, valid, inv_s=1.0):
    """a_n * u_n * inv_s for valid rows, exactly 0 for the others"""
    a = np.asarray(a, np.float64)
    valid = np.asarray(valid, bool)
    u = np.where(valid, np.asarray(upstream, np.float64).reshape(-1), 0.0)
    out = a * (u * inv_s)[:, None]
    out[~valid] = 0.0
    return out


def linear_cross_entropy(x, w, b, targets, upstream, ignore_index=None):
    """(rows, dx, dW, dbias) in float64 of the rows of cross_entropy(x @ w + b) under the upstream vector"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    z = x64 @ w64
    if b is not None:
        z = z + np.asarray(b, np.float64).reshape(-1)
    d = dlogits(z, targets, upstream, ignore_index)
    return rows(z, targets, ignore_index), d @ w64.T, x64.T @ d, d.sum(0)
