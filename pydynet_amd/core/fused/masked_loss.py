"""Cross entropy with `ignore_index`, stated once in float64 array arithmetic.

This module is the contract of the masked kernels in csrc/masked_loss.hip (entries of include/pdn_loss.h, prefix pdnl_),
as optim/clip.py and llm/penalties.py are for theirs; the emulator part and the tests compare against it.  The
reference's cross entropy (nn/functional.py:364-381) has no `ignore_index`: this is an extension.

    valid_n = (t_n != ignore_index)                 ignore_index is any int64, an id inside [0, V) included
    row_n   = logsumexp(z_n) - z_n[t_n]             for valid rows; an ignored row adds 0
    count   = sum(valid)
    'sum'   : loss = sum(row[valid])                                 dz_n = (softmax(z_n) - onehot(t_n)) * g
    'mean'  : loss = sum(row[valid]) / count                         dz_n = (softmax(z_n) - onehot(t_n)) * g / count
    dz_n    = 0.0 exactly for every ignored row -- it adds nothing to dx (that row of dx is exactly 0), dW or dbias
    count == 0: loss = 0 and every gradient is 0

torch returns NaN for the mean over no rows.  A training step that is captured once and replayed over changing targets
cannot look at the loss before the optimizer runs, and one NaN gradient would stay in Adam's moments for good; an all-padding
batch therefore is a step with zero gradient.

A target that is neither `ignore_index` nor inside [0, V) is an error (the device raises its error flag); negative targets do
not wrap in the masked form.

Data parallel: each rank divides by its own count and the gradients are then averaged over the ranks, which is the mean
over all valid tokens only when the ranks hold equally many of them.
"""
import numpy as np


def valid_rows(targets, ignore_index):
    return np.asarray(targets).reshape(-1) != int(ignore_index)


def check_targets(targets, ignore_index, V):
    """IndexError for a target that is neither `ignore_index` nor a class."""
    t = np.asarray(targets).reshape(-1)
    bad = valid_rows(t, ignore_index) & ((t < 0) | (t >= V))
    if bad.any():
        raise IndexError(f"cross entropy target {int(t[bad][0])} is neither ignore_index nor inside [0, {V})")


def scale(targets, ignore_index, reduction):
    """(count, factor) with factor = 1/count under 'mean' (0 when no row remains) and 1 under 'sum'."""
    count = int(valid_rows(targets, ignore_index).sum())
    if reduction == "sum":
        return count, 1.0
    return count, (1.0 / count if count else 0.0)


def cross_entropy(logits, targets, ignore_index, reduction="mean", upstream=1.0):
    """(loss, dlogits) in float64 for (rows, V) logits."""
    z = np.asarray(logits, np.float64)
    t = np.asarray(targets).reshape(-1)
    rows, V = z.shape
    check_targets(t, ignore_index, V)
    valid = valid_rows(t, ignore_index)
    ts = np.where(valid, t, 0)
    m = z.max(-1, keepdims=True)
    lse = np.log(np.exp(z - m).sum(-1, keepdims=True)) + m
    per_row = np.where(valid, lse[:, 0] - z[np.arange(rows), ts], 0.0)
    _, factor = scale(t, ignore_index, reduction)
    d = np.exp(z - lse)
    d[np.arange(rows), ts] -= 1.0
    d *= float(upstream) * factor
    d[~valid] = 0.0
    return float(per_row.sum() * factor), d


def linear_cross_entropy(x, w, b, targets, ignore_index, reduction="mean", upstream=1.0):
    """(loss, dx, dW, dbias) in float64 of cross_entropy(x @ w + b)."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    z = x64 @ w64
    if b is not None:
        z = z + np.asarray(b, np.float64).reshape(-1)
    loss, d = cross_entropy(z, targets, ignore_index, reduction, upstream)
    return loss, d @ w64.T, x64.T @ d, d.sum(0)
