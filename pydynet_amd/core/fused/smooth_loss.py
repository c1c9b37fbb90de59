"""Cross entropy with `label_smoothing` and `z_loss`, stated once in float64 array arithmetic.

This module is the contract of the kernels in csrc/smooth_loss.hip (entries of include/pdn_smoothloss.h, prefix pdnz_), as
masked_loss.py and row_loss.py are for theirs; the emulator part and the tests compare against it.  The reference's cross
entropy (nn/functional.py:364-381) has neither argument: this is an extension.

    eps = label_smoothing in [0, 1]      the target distribution is (1 - eps) onehot(t_n) + eps / V
    lam = z_loss >= 0                    adds lam * logsumexp(z_n)^2 per row (the PaLM auxiliary term)
    valid_n = ignore_index is None or t_n != ignore_index
    lse_n   = logsumexp(z_n),  p = softmax(z_n),  a_n = 1 + 2 lam lse_n
    row_n   = lse_n - (1 - eps) z_n[t_n] - eps mean_v(z_n) + lam lse_n^2      for valid rows, 0 for ignored ones
    dz_n    = u_n (a_n p - (1 - eps) onehot(t_n) - eps / V)                   for valid rows, 0.0 exactly for ignored ones
            = u'_n (p - onehot(t_n)) + c_n onehot(t_n) - e_n                  u' = u a,  c = u (2 lam lse + eps),  e = u eps / V

    'none' : the value is row (rows,), u the (rows,) upstream vector; an ignored row's dz is 0 WHATEVER u_n holds (NaN too)
    'sum'  : loss = sum(row),          u_n = g          (g: the upstream scalar)
    'mean' : loss = sum(row) / count,  u_n = g / count  (count: rows that remain; count == 0: loss 0, every gradient 0) --
             the z-loss and the smoothing term are averaged over the same remaining rows as the cross entropy itself

The decomposition in the last line of dz is what the lm_head node is built on: the first term is the backward of the
reduction='none' node as it is (core/fused/row_loss.py) under the upstream vector u'; the second touches one column per
row; the third is the same number in every column of a row (rank 1).  Neither needs a pass over the logits:

    mean_v z_n = x_n . wsum / V + bsum / V                  wsum[k] = sum_v W[k, v],  bsum = sum_v b[v]
    dx_n  += c_n W[:, t_n] - e_n wsum
    dW[:, v] += sum_{n: t_n = v} c_n x_n - sum_n e_n x_n
    db[v]    += sum_{n: t_n = v} c_n     - sum_n e_n

A valid target outside [0, V) is an error (IndexError here, the error flag on the device); negative targets do not wrap.
eps == 0 and lam == 0 is NOT a case of this module: every layer below then takes exactly the path it took before.
"""
import numpy as np

from . import row_loss


def check_arguments(label_smoothing, z_loss):
    """(eps, lam) as floats; ValueError outside eps in [0, 1], lam >= 0"""
    eps, lam = float(label_smoothing), float(z_loss)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must lie in [0, 1], got {label_smoothing}")
    if not lam >= 0.0:
        raise ValueError(f"z_loss must be >= 0, got {z_loss}")
    return eps, lam


def _lse(z):
    m = z.max(-1, keepdims=True)
    return (np.log(np.exp(z - m).sum(-1, keepdims=True)) + m)[:, 0]


def _prepare(logits, targets, ignore_index):
    z = np.asarray(logits, np.float64)
    t = np.asarray(targets).reshape(-1)
    row_loss.check_targets(t, ignore_index, z.shape[1])
    valid = row_loss.valid_rows(t, ignore_index)
    return z, np.where(valid, t, 0), valid


def rows(logits, targets, label_smoothing=0.0, z_loss=0.0, ignore_index=None):
    """the 'none' node's value: (rows,) float64, 0 at ignored rows"""
    eps, lam = check_arguments(label_smoothing, z_loss)
    z, ts, valid = _prepare(logits, targets, ignore_index)
    lse = _lse(z)
    r = lse - (1.0 - eps) * z[np.arange(len(ts)), ts] - eps * z.mean(-1) + lam * lse * lse
    return np.where(valid, r, 0.0)


def coefficients(lse, valid, upstream, label_smoothing, z_loss, V):
    """(u', c, e): the three row coefficient vectors of the decomposition, exactly 0 on ignored rows"""
    eps, lam = check_arguments(label_smoothing, z_loss)
    valid = np.asarray(valid, bool)
    u = np.where(valid, np.broadcast_to(np.asarray(upstream, np.float64), valid.shape), 0.0)
    l = np.where(valid, np.asarray(lse, np.float64), 0.0)
    return u * (1.0 + 2.0 * lam * l), u * (2.0 * lam * l + eps), u * (eps / V)


def dlogits(logits, targets, upstream, label_smoothing=0.0, z_loss=0.0, ignore_index=None):
    """(rows, V) float64 gradient of sum_n u_n row_n, the direct formula; ignored rows are 0 by a select"""
    eps, lam = check_arguments(label_smoothing, z_loss)
    z, ts, valid = _prepare(logits, targets, ignore_index)
    n, V = z.shape
    u = np.where(valid, np.broadcast_to(np.asarray(upstream, np.float64), (n,)), 0.0)
    lse = _lse(z)
    d = np.exp(z - lse[:, None]) * (1.0 + 2.0 * lam * lse)[:, None]
    d[np.arange(n), ts] -= 1.0 - eps
    d -= eps / V
    d *= u[:, None]
    d[~valid] = 0.0
    return d


def dlogits_decomposed(logits, targets, upstream, label_smoothing=0.0, z_loss=0.0, ignore_index=None):
    """the same gradient as the three terms the lm_head node forms: the 'none' backward under u', the target-column term
    and the uniform term"""
    z, ts, valid = _prepare(logits, targets, ignore_index)
    n, V = z.shape
    up, c, e = coefficients(_lse(z), valid, upstream, label_smoothing, z_loss, V)
    d = row_loss.dlogits(z, np.where(valid, ts, -1), up, -1)
    d[np.arange(n), ts] += c
    d -= e[:, None]
    d[~valid] = 0.0
    return d


def _factor(targets, ignore_index, reduction):
    if reduction not in ("mean", "sum"):
        raise ValueError("reduction must be mean, sum or none.")
    t = np.asarray(targets).reshape(-1)
    count = int(row_loss.valid_rows(t, ignore_index).sum())
    return 1.0 if reduction == "sum" else (1.0 / count if count else 0.0)


def value(logits, targets, label_smoothing=0.0, z_loss=0.0, ignore_index=None, reduction="mean"):
    """the node's value alone: the (rows,) vector under 'none', else a float"""
    r = rows(logits, targets, label_smoothing, z_loss, ignore_index)
    return r if reduction == "none" else float(r.sum() * _factor(targets, ignore_index, reduction))


def cross_entropy(logits, targets, label_smoothing=0.0, z_loss=0.0, ignore_index=None, reduction="mean", upstream=1.0):
    """(loss, dlogits) in float64 for (rows, V) logits; 'none': loss is the (rows,) vector and `upstream` a (rows,) vector,
    'mean' / 'sum': a float and `upstream` a scalar"""
    u = upstream if reduction == "none" else float(upstream) * _factor(targets, ignore_index, reduction)
    return (value(logits, targets, label_smoothing, z_loss, ignore_index, reduction),
            dlogits(logits, targets, u, label_smoothing, z_loss, ignore_index))


def weight_sums(w, b):
    """(wsum, bsum): the row sums of W over the vocabulary and the sum of the bias (0 without one)"""
    return np.asarray(w, np.float64).sum(1), (float(np.asarray(b, np.float64).sum()) if b is not None else 0.0)


def linear_cross_entropy(x, w, b, targets, label_smoothing=0.0, z_loss=0.0, ignore_index=None, reduction="mean",
                         upstream=1.0):
    """(value, dx, dW, dbias) in float64 of cross_entropy(x @ w + b) with the two terms"""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    z = x64 @ w64
    if b is not None:
        z = z + np.asarray(b, np.float64).reshape(-1)
    value, d = cross_entropy(z, targets, label_smoothing, z_loss, ignore_index, reduction, upstream)
    return value, d @ w64.T, x64.T @ d, d.sum(0)

