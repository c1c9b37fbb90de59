"""Plain float64 NumPy statements of the reference program's formulas, shared by tests/test_generic_kernels.py.

Nothing here touches this package: every function is NumPy on host arrays, written from the formula each kernel cites
(include/pdn_hip.h names the call sites), so a kernel and its emulation are both judged by a third, independent statement."""
import numpy as np

F64 = np.float64


# ---- pooling / im2col / col2im (pydynet/nn/functional.py:194-339) --------------------------------------------------
def out_size(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def windows(x, k, s, p):
    """(N, C, k, k, oh, ow): entry [n, c, i, j, oy, ox] = padded x[n, c, oy*s + i, ox*s + j] (a copy, one slice per tap)."""
    N, C, H, W = x.shape
    oh, ow = out_size(H, W, k, s, p)
    xp = np.pad(x, [(0, 0), (0, 0), (p, p), (p, p)])
    win = np.empty((N, C, k, k, oh, ow), x.dtype)
    for i in range(k):
        for j in range(k):
            win[:, :, i, j] = xp[:, :, i:i + s * (oh - 1) + 1:s, j:j + s * (ow - 1) + 1:s]
    return win


def scatter_windows(contrib, H, W, k, s, p):
    """The adjoint of `windows` (xp.add.at on the overlapping view, functional.py:224-232): contrib (N, C, k, k, oh, ow)."""
    N, C, _, _, oh, ow = contrib.shape
    dxp = np.zeros((N, C, H + 2 * p, W + 2 * p), contrib.dtype)
    for i in range(k):
        for j in range(k):
            dxp[:, :, i:i + s * (oh - 1) + 1:s, j:j + s * (ow - 1) + 1:s] += contrib[:, :, i, j]
    return dxp[:, :, p:p + H, p:p + W]


def pool_fwd(x, k, s, p, mode):
    win = windows(x.astype(F64), k, s, p)
    return win.max((2, 3)) if mode == "max" else win.mean((2, 3))


def pool_bwd(x, dy, k, s, p, mode):
    """max: EVERY position equal to its window's maximum receives the window's gradient (tensor.py:744-750), the padding
    zeros included (they are cropped afterwards); avg: g / k^2 to every position."""
    N, C, H, W = x.shape
    win = windows(x.astype(F64), k, s, p)
    g = dy.astype(F64)[:, :, None, None]
    if mode == "max":
        contrib = (win == win.max((2, 3), keepdims=True)) * g
    else:
        contrib = np.broadcast_to(g / (k * k), win.shape)
    return scatter_windows(np.ascontiguousarray(contrib), H, W, k, s, p)


def tie_census(x, k, s, p):
    """(#windows with two or more maxima, #windows that reach the padding and that ONLY the padding's zero wins: every
    value of the image inside them, if any, is below 0)."""
    win = windows(x.astype(F64), k, s, p)
    tied = int(((win == win.max((2, 3), keepdims=True)).sum((2, 3)) >= 2).sum())
    inside = windows(np.ones(x.shape), k, s, p) == 1                  # True on the image, False on the padding
    best_inside = np.where(inside, win, -np.inf).max((2, 3))
    pad_wins = int(((~inside).any((2, 3)) & (best_inside < 0)).sum())
    return tied, pad_wins


def conv2d_ref(x, w, b, g, s, p):
    """y, dx, dw, db of conv2d (functional.py:254-281) and of sum(y * g), float64."""
    x, w, g = x.astype(F64), w.astype(F64), g.astype(F64)
    N, C, H, W = x.shape
    O, _, k, _ = w.shape
    win = windows(x, k, s, p)                                          # (N, C, k, k, oh, ow)
    oh, ow = win.shape[-2:]
    y = np.einsum("ncijyx,ocij->noyx", win, w)
    if b is not None:
        y = y + b.astype(F64).reshape(1, O, 1, 1)
    dw = np.einsum("ncijyx,noyx->ocij", win, g)
    db = g.sum((0, 2, 3))
    dx = scatter_windows(np.einsum("noyx,ocij->ncijyx", g, w), H, W, k, s, p)
    return y, dx, dw, db


# ---- gates (core/tensor.py:999-1003, 1012-1016: the same functions, float64 has no need of the piecewise form) -------
def sigmoid(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(v, F64)))


def lstm_cell(lin, c):
    """nn/modules/rnn.py:244-262 -> gates [f | i | o | tanh g], tanh(c'), h', c'."""
    lin, c = lin.astype(F64), c.astype(F64)
    H = c.shape[1]
    f, i, o = (sigmoid(lin[:, j * H:(j + 1) * H]) for j in range(3))
    g = np.tanh(lin[:, 3 * H:])
    cn = f * c + i * g
    t = np.tanh(cn)
    return np.concatenate([f, i, o, g], 1), t, o * t, cn


def lstm_cell_bwd(dh, dcn, gates, t, c):
    """Gradients of the pre-activations (B, 4H) and of c, given dh' and the dc' that later consumers add."""
    gates, t, c, dh, dcn = (a.astype(F64) for a in (gates, t, c, dh, dcn))
    H = c.shape[1]
    f, i, o, g = (gates[:, j * H:(j + 1) * H] for j in range(4))
    dc = dcn + dh * o * (1 - t * t)
    dlin = np.concatenate([dc * c * f * (1 - f), dc * g * i * (1 - i), dh * t * o * (1 - o), dc * i * (1 - g * g)], 1)
    return dlin, dc * f


def lstm_sequence(x, wx, wh, b, wo, whn, wcn):
    """nn.LSTM, one layer, zero initial state; loss = sum(out * wo) + sum(hn * whn) + sum(cn * wcn).
    Returns out, hn, cn and the gradients dx, dWx, dWh, db."""
    x, wx, wh, b, wo, whn, wcn = (a.astype(F64) for a in (x, wx, wh, b, wo, whn, wcn))
    T, B, _ = x.shape
    H = wh.shape[0]
    h, c = np.zeros((B, H)), np.zeros((B, H))
    saved, outs = [], []
    for t in range(T):
        gates, tc, hn, cn = lstm_cell(x[t] @ wx + h @ wh + b, c)
        saved.append((h, c, gates, tc))
        h, c = hn, cn
        outs.append(h)
    out = np.stack(outs)
    dx, dwx, dwh, db = np.zeros_like(x), np.zeros_like(wx), np.zeros_like(wh), np.zeros_like(b)
    dh, dc = whn.reshape(B, H).copy(), wcn.reshape(B, H).copy()
    for t in range(T - 1, -1, -1):
        hp, cp, gates, tc = saved[t]
        dlin, dc = lstm_cell_bwd(dh + wo[t], dc, gates, tc, cp)
        dx[t] = dlin @ wx.T
        dwx += x[t].T @ dlin
        dwh += hp.T @ dlin
        db += dlin.sum(0)
        dh = dlin @ wh.T
    return out, h, c, dx, dwx, dwh, db


def rnn_sequence(x, wx, wh, b, wo, act):
    """nn.RNN, one layer, zero initial state (rnn.py:35-47); loss = sum(out * wo).  relu' = [out == lin]."""
    x, wx, wh, b, wo = (a.astype(F64) for a in (x, wx, wh, b, wo))
    T, B, _ = x.shape
    H = wh.shape[0]
    h = np.zeros((B, H))
    saved, outs = [], []
    for t in range(T):
        lin = x[t] @ wx + h @ wh + b
        y = np.tanh(lin) if act == "tanh" else np.maximum(0.0, lin)
        saved.append((h, lin, y))
        h = y
        outs.append(h)
    dx, dwx, dwh, db = np.zeros_like(x), np.zeros_like(wx), np.zeros_like(wh), np.zeros_like(b)
    dh = np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        hp, lin, y = saved[t]
        d = dh + wo[t]
        dlin = (1 - y * y) * d if act == "tanh" else (y == lin) * d
        dx[t] = dlin @ wx.T
        dwx += x[t].T @ dlin
        dwh += hp.T @ dlin
        db += dlin.sum(0)
        dh = dlin @ wh.T
    return np.stack(outs), h, dx, dwx, dwh, db


def gru_sequence(x, h0, wx1, wh1, wx2, wh2, b1, b2, wo):
    """The reference's GRU (rnn.py:537-544; NOT PyTorch's: r multiplies h BEFORE the Wh2 product, z weights the candidate):
        [z, r] = sigmoid(x Wx1 + h Wh1 + b1);  n = tanh(x Wx2 + (r h) Wh2 + b2);  h' = (1 - z) h + z n
    loss = sum(out * wo).  Returns out and the gradients in the order x, h0, wx1, wh1, wx2, wh2, b1, b2."""
    x, h0, wx1, wh1, wx2, wh2, b1, b2, wo = (a.astype(F64) for a in (x, h0, wx1, wh1, wx2, wh2, b1, b2, wo))
    T, B, _ = x.shape
    H = h0.shape[1]
    h, saved, outs = h0, [], []
    for t in range(T):
        a1 = sigmoid(x[t] @ wx1 + h @ wh1 + b1)
        z, r = a1[:, :H], a1[:, H:]
        rh = r * h
        n = np.tanh(x[t] @ wx2 + rh @ wh2 + b2)
        saved.append((h, z, r, rh, n))
        h = (1 - z) * h + z * n
        outs.append(h)
    grads = [np.zeros_like(a) for a in (x, h0, wx1, wh1, wx2, wh2, b1, b2)]
    dx, _, dwx1, dwh1, dwx2, dwh2, db1, db2 = grads
    dh = np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        hp, z, r, rh, n = saved[t]
        d = dh + wo[t]
        da2 = d * z * (1 - n * n)
        drh = da2 @ wh2.T
        da1 = np.concatenate([d * (n - hp) * z * (1 - z), drh * hp * r * (1 - r)], 1)
        dh = d * (1 - z) + drh * r + da1 @ wh1.T
        dx[t] = da1 @ wx1.T + da2 @ wx2.T
        dwx1 += x[t].T @ da1; dwh1 += hp.T @ da1; dwx2 += x[t].T @ da2; dwh2 += rh.T @ da2
        db1 += da1.sum(0); db2 += da2.sum(0)
    grads[1] = dh
    return np.stack(outs), grads


# ---- last-axis LayerNorm (llm/clip/model.py:66-80) and the gated sigmoid (:92-95) -----------------------------------
def layernorm_stats(x, eps):
    x = x.astype(F64)
    mu = x.mean(-1)
    return mu, 1.0 / np.sqrt(np.square(x - mu[..., None]).mean(-1) + eps)


def layernorm_fwd(x, w, b, mu, rstd):
    return (x.astype(F64) - np.asarray(mu, F64)[..., None]) * np.asarray(rstd, F64)[..., None] * w.astype(F64) + b.astype(F64)


def layernorm_bwd(x, w, mu, rstd, dy):
    """dx, dw, db of y = xhat * w + b with xhat = (x - mu) * rstd, mu and rstd the row statistics."""
    x, w, dy = x.astype(F64), w.astype(F64), dy.astype(F64)
    rs = np.asarray(rstd, F64)[..., None]
    xh = (x - np.asarray(mu, F64)[..., None]) * rs
    dz = dy * w
    dx = (dz - dz.mean(-1, keepdims=True) - xh * (dz * xh).mean(-1, keepdims=True)) * rs
    lead = tuple(range(x.ndim - 1))
    return dx, (dy * xh).sum(lead), dy.sum(lead)


def gated_sigmoid(x, a):
    x = x.astype(F64)
    s = sigmoid(a * x)
    return x * s, s * (1 + a * x * (1 - s))


# ---- float64 products ----------------------------------------------------------------------------------------------
def gemm_longdouble(a, b, c0, alpha, beta):
    """alpha * a @ b + beta * c0 in np.longdouble, and the componentwise rounding bound of ANY length-K inner product
    evaluated in float64, in any order, with or without FMA:  (K + 2) * 2^-53 * (|alpha| |a| @ |b| + |beta| |c0|)."""
    K = a.shape[-1]
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    ref = alpha * np.matmul(al, bl)
    mag = abs(alpha) * np.matmul(np.abs(al), np.abs(bl))
    if beta != 0:
        ref = ref + beta * c0.astype(np.longdouble)
        mag = mag + abs(beta) * np.abs(c0.astype(np.longdouble))
    return ref, (K + 2) * 2.0 ** -53 * mag
