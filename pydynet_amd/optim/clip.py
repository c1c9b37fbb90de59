"""Global-norm gradient clipping and the Adam update that consumes it, stated once in array arithmetic.

This module is the contract of the fused kernels in csrc/optim.hip (as llm/penalties.py and llm/logprobs.py are for
theirs) AND the path every parameter takes that the kernels do not cover: the `cpu` device, float64 parameters,
non-contiguous gradients.  The reference has no counterpart.

    norm   = |s| * sqrt(sum over all tensors of sum(g.astype(float64)**2))      one global 2-norm, s = grad_scale
    finite = isfinite(norm)
    coef   = min(1, max_norm / (norm + 1e-6)) if finite else 0                   max_norm None / inf -> 1

Adam with the coefficient: the package's Adam arithmetic (the reference's, eps outside the bias correction) with
`g*s` replaced by `g*s*coef`; gradients in memory are not rewritten; when `finite` is false the whole update is
skipped.  Decoupled decay: first `p -= lr*wd*p` (the plain rate, not lr*a_t), then the update without `wd*p` in the
gradient -- "the reference's Adam with the decay decoupled", not a bit-copy of PyTorch's AdamW.
"""
from math import isfinite, sqrt

import numpy as np

NORM_EPS = 1e-6


def sum_of_squares(grads):
    """sum over tensors of sum(g.astype(float64)**2) as a Python float; NumPy or device arrays (one read-back each)."""
    total = 0.0
    for g in grads:
        if g is None:
            continue
        g64 = g.astype(np.float64)
        total += float((g64 * g64).sum())
    return total


def total_norm(grads, grad_scale=1.0):
    return abs(float(grad_scale)) * sqrt(sum_of_squares(grads)) if grads else 0.0


def coefficient(norm, max_norm):
    """(coef, finite) for a norm; `max_norm` None, inf or <= 0 only measures (coef 1 unless the norm is not finite)."""
    finite = isfinite(norm)
    if not finite:
        return 0.0, False
    if max_norm is None or max_norm <= 0:
        return 1.0, True
    return min(1.0, float(max_norm) / (norm + NORM_EPS)), True


def adam_update(p, g, m, v, step, lr_wd, beta1, beta2, eps, weight_decay, scale, decoupled):
    """One parameter's update in place, in the arrays' own dtype.  `scale` = grad_scale * coef and `step` = lr * a_t are
    Python floats (a NumPy float64 scalar would promote float32 arrays)."""
    grad = g * scale if scale != 1.0 else g
    if decoupled:
        p -= lr_wd * p
    else:
        grad = grad + weight_decay * p
    m *= beta1
    m += (1 - beta1) * grad
    v *= beta2
    v += (1 - beta2) * grad ** 2
    p -= step * m / (v ** 0.5 + eps)
