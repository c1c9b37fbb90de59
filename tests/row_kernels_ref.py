"""Plain NumPy statements of the row, loss, embedding, reduction and optimizer operations behind csrc/fused.hip and
csrc/reduce.hip, for tests/test_row_kernels.py.  Nothing here imports the package under test.

Every function takes a `dtype`: float64 (the default) is the reference a kernel is held to; float32 evaluates the SAME
statement in the kernels' own number format, which measures the error that statement has in fp32 whatever the kernel does
(the yardstick of the large-offset and wide-spread cases, where that error exceeds the usual stream tolerance)."""
import numpy as np


def _f(a, dtype):
    return np.asarray(a).astype(dtype)


# -- softmax ----------------------------------------------------------------------------------------------------------
def causal_keep(rows, cols, causal_L, start_pos):
    """Which (row, column) pairs take part: column c of row r is kept while c <= r % causal_L + start_pos."""
    if causal_L <= 0:
        return np.ones((rows, cols), bool)
    return np.arange(cols)[None, :] <= (np.arange(rows) % causal_L)[:, None] + start_pos


def softmax_fwd(x, divisor=1.0, causal_L=0, start_pos=0, dtype=np.float64):
    """y = softmax(x / divisor) over the kept columns of each row; the others are exactly 0."""
    x = _f(x, dtype)
    keep = causal_keep(x.shape[0], x.shape[1], causal_L, start_pos)
    a = np.where(keep, x / dtype(divisor), dtype(-np.inf))
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_bwd(y, dy, divisor=1.0, dtype=np.float64):
    """dx = (dy - sum(dy * y)) * y / divisor"""
    y, dy = _f(y, dtype), _f(dy, dtype)
    return (dy - (dy * y).sum(-1, keepdims=True)) * y / dtype(divisor)


# -- RMSNorm ----------------------------------------------------------------------------------------------------------
def rmsnorm_fwd(x, w, eps, dtype=np.float64):
    """rms = sqrt(mean(x^2) + eps); y = x / rms * w.  Returns (y, rms)."""
    x, w = _f(x, dtype), _f(w, dtype)
    rms = np.sqrt((x * x).mean(-1) + dtype(eps))
    return x / rms[:, None] * w, rms


def rmsnorm_bwd(x, w, rms, dy, dx_residual=None, dtype=np.float64):
    """z = x / rms; dz = dy * w; dx = (dz - z * mean(z * dz)) / rms (+ dx_residual); dw = sum over rows of dy * z."""
    x, w, rms, dy = _f(x, dtype), _f(w, dtype), _f(rms, dtype)[:, None], _f(dy, dtype)
    z, dz = x / rms, dy * w
    dx = (dz - z * (z * dz).mean(-1, keepdims=True)) / rms
    if dx_residual is not None:
        dx = dx + _f(dx_residual, dtype)
    return dx, (dy * z).sum(0)


# -- cross entropy ----------------------------------------------------------------------------------------------------
def wrap(idx, n):
    """NumPy's index rule: a negative index counts from the end."""
    idx = np.asarray(idx, np.int64)
    return np.where(idx < 0, idx + n, idx)


def cross_entropy(x, t, gscale=1.0, mean=True, dtype=np.float64):
    """lse = log sum exp (shifted by the row maximum), loss_row = lse - x[t], loss = mean or sum of the rows,
    dlogits = (exp(x - lse) - onehot(t)) * gscale.  Returns (loss_row, lse, loss, dlogits)."""
    x = _f(x, dtype)
    rows, V = x.shape
    t = wrap(t, V)
    m = x.max(-1, keepdims=True)
    lse = (np.log(np.exp(x - m).sum(-1, keepdims=True)) + m)[:, 0]
    loss_row = lse - x[np.arange(rows), t]
    d = np.exp(x - lse[:, None])
    d[np.arange(rows), t] -= 1
    return loss_row, lse, (loss_row.mean() if mean else loss_row.sum()), d * dtype(gscale)


# -- SiLU / SwiGLU ----------------------------------------------------------------------------------------------------
def swiglu_fwd(g, u=None, dtype=np.float64):
    """silu(g) = g / (1 + exp(-g)); y = silu(g) (* u)"""
    g = _f(g, dtype)
    with np.errstate(over="ignore"):
        y = g / (1 + np.exp(-g))
    return y if u is None else y * _f(u, dtype)


def swiglu_bwd(g, u, dy, dtype=np.float64):
    """s = sigmoid(g); dg = dy (* u) * s * (1 + g * (1 - s)); du = dy * silu(g).  Returns (dg, du or None)."""
    g, dy = _f(g, dtype), _f(dy, dtype)
    with np.errstate(over="ignore"):
        s = 1 / (1 + np.exp(-g))
    dg = dy * s * (1 + g * (1 - s))
    if u is None:
        return dg, None
    return dg * _f(u, dtype), dy * g * s


# -- RoPE -------------------------------------------------------------------------------------------------------------
def rope(x, cos, sin, L, sign=1.0, dtype=np.float64):
    """x (rows, heads, hd) as interleaved pairs; row r sits at position r % L of the (L, hd / 2) tables:
    y[2i] = x[2i] cos - sign x[2i+1] sin;  y[2i+1] = sign x[2i] sin + x[2i+1] cos"""
    x = _f(x, dtype)
    pos = np.arange(x.shape[0]) % L
    c, s = _f(cos, dtype)[pos][:, None, :], dtype(sign) * _f(sin, dtype)[pos][:, None, :]
    y = np.empty_like(x)
    y[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
    y[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
    return y


# -- embedding --------------------------------------------------------------------------------------------------------
def scatter(dW, g, ids, mode, row_owner=None, owner_tag=0.0):
    """The gradient of a gather, into a copy of dW, in the dtype of dW.  Ids wrap as NumPy's do; ids outside the table
    are dropped.  mode 0: full[ids] = g (the LAST row holding an id wins), written over those rows of dW; mode 1: dW += full;
    mode 2: np.add.at(dW, ids, g), every occurrence.  row_owner: only table rows tagged owner_tag are touched (the last
    occurrence is found first, over all rows, and the filter applied to it)."""
    out = np.array(dW)
    V = out.shape[0]
    ids = wrap(ids, V)
    ok = (ids >= 0) & (ids < V)
    rows = np.flatnonzero(ok)
    if mode == 2:
        if row_owner is not None:
            rows = rows[np.asarray(row_owner)[ids[rows]] == owner_tag]
        np.add.at(out, ids[rows], np.asarray(g)[rows].astype(out.dtype))
        return out
    last = {}
    for r in rows:
        last[int(ids[r])] = int(r)
    for i, r in last.items():
        if row_owner is not None and row_owner[i] != owner_tag:
            continue
        out[i] = g[r] if mode == 0 else out[i] + g[r].astype(out.dtype)
    return out


# -- Adam -------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, b1, b2, eps, wd, grad_scale, dtype=np.float64):
    """g' = g * grad_scale + wd * p; m = b1 m + (1 - b1) g'; v = b2 v + (1 - b2) g'^2; p -= step * m / (sqrt(v) + eps)"""
    p, g, m, v = (_f(a, dtype) for a in (p, g, m, v))
    gg = g * dtype(grad_scale) + dtype(wd) * p
    m = m * dtype(b1) + (1 - dtype(b1)) * gg
    v = v * dtype(b2) + (1 - dtype(b2)) * gg * gg
    return p - dtype(step) * m / (np.sqrt(v) + dtype(eps)), m, v


def adam_step_size(lr, b1, b2, t):
    """lr * sqrt(1 - b2^t) / (1 - b1^t)"""
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
