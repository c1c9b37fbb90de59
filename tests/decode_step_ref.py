"""Plain float64 NumPy statements of the operations of the graph-replayed decode step (csrc/decode.hip, decode_stage.h),
shared by tests/test_decode_step_variants.py.

Nothing here touches this package: every function is NumPy on host arrays, written from the formula the kernel cites
(llm/llama/model.py:47-58, 105-121, 254-269 and norm.py:245-248 of the reference program), so a kernel and its emulation
are both judged by a third, independent statement."""
import numpy as np

F64 = np.float64


# ---- the staged input row: f(x) ---------------------------------------------------------------------------------------
def rmsnorm(x, w, eps):
    """x / sqrt(mean(x^2) + eps) * w over the last axis (norm.py:245-248)."""
    x = np.asarray(x, F64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + F64(eps)) * np.asarray(w, F64)


def swiglu(gu, K):
    """silu(gate) * up on packed [gate | up] rows of width 2 K (functional.py:39-40, model.py:56-58)."""
    g, u = np.asarray(gu[..., :K], F64), np.asarray(gu[..., K:2 * K], F64)
    with np.errstate(over="ignore"):                 # (exp(-g) = inf in float32 terms is a quotient of 0 here as well)
        return g / (1.0 + np.exp(-g)) * u


def merge(rec):
    """Flash-decoding merge of (..., ns, H, 4 + hd) records [m, l, -, - | sum of exp(s - m) v] over the ns key ranges:
         att[h] = sum_s exp(m_s - M) o_s / sum_s exp(m_s - M) l_s,   M = max over the ranges with keys (l > 0).
    A range without keys has no say: neither its m nor its sums are read.  Returns (..., H * hd)."""
    rec = np.asarray(rec, F64)
    m, l, o = rec[..., 0], rec[..., 1], rec[..., 4:]
    live = l > 0
    M = np.where(live, m, -np.inf).max(-2, keepdims=True)
    e = np.where(live, np.exp(np.where(live, m, 0.0) - M), 0.0)
    num = np.where(live[..., None], e[..., None] * np.where(live[..., None], o, 0.0), 0.0).sum(-3)
    att = num / (e * np.where(live, l, 0.0)).sum(-2)[..., None]
    return att.reshape(att.shape[:-2] + (-1,))


def handoff(base, parts):
    """base (B, K) + sum over the partial rows parts (B, n_parts, K) -- the hand-off of decode_stage.h."""
    return np.asarray(base, F64) + np.asarray(parts, F64).sum(1)


# ---- the product ------------------------------------------------------------------------------------------------------
def gemv(a, blocks, bias=None, residual=None):
    """y = a @ [W_0 | W_1 | ...] + bias + residual; blocks: the (K, blk_cols) column blocks in order."""
    a = np.asarray(a, F64)
    y = np.concatenate([a @ np.asarray(Wj, F64) for Wj in blocks], axis=1)
    if bias is not None:
        y = y + np.asarray(bias, F64)
    if residual is not None:
        y = y + np.asarray(residual, F64)
    return y


# ---- the greedy pick --------------------------------------------------------------------------------------------------
def tile_width(N):
    """Columns per workgroup of pdn_decode_gemv_f32, hence per candidate (pdn_decode_gemv_blocks: 16 / 32 / 64)."""
    return 16 if N <= 4096 else (32 if N <= 16384 else 64)


def n_tiles(N):
    return -(-N // tile_width(N))


def candidate_tables(y):
    """Per row and per workgroup: the maximum of the workgroup's columns and the FIRST column that holds it
    (B, n_tiles) each; the last workgroup may own fewer columns."""
    B, N = y.shape
    tn, nt = tile_width(N), n_tiles(N)
    v, a = np.empty((B, nt), F64), np.empty((B, nt), np.int64)
    for j in range(nt):
        seg = y[:, j * tn:min(N, (j + 1) * tn)]
        v[:, j] = seg.max(-1)
        a[:, j] = j * tn + np.array([int(np.flatnonzero(r == r.max())[0]) for r in seg])
    return v, a


def pick(vals, args):
    """Per row: among the candidates with the largest value, the lowest column -- whatever order they come in."""
    return np.array([int(a[v == v.max()].min()) for v, a in zip(vals, args)], np.int64)


def first_argmax(z):
    """Per row the first index of the maximum (model.py:262-268: argmax); a row of NaNs picks 0."""
    out = np.zeros(len(z), np.int64)
    for b, r in enumerate(z):
        if not np.isnan(r).all():
            out[b] = int(np.flatnonzero(r == np.nanmax(r))[0])
    return out


# ---- one decode-attention row (model.py:23-44, 105-121 with one new token) -----------------------------------------------
def rope(v, c, s):
    """Rotate interleaved pairs (v[2i], v[2i+1]) of (..., hd) by the angles with cos c / sin s (hd / 2 each)."""
    a = np.asarray(v, F64).reshape(v.shape[:-1] + (v.shape[-1] // 2, 2))
    out = np.empty_like(a)
    out[..., 0] = a[..., 0] * c - a[..., 1] * s
    out[..., 1] = a[..., 0] * s + a[..., 1] * c
    return out.reshape(v.shape)


def attention_row(qkv, kc, vc, cos, sin, pos, H):
    """qkv (3 D,) packed [q | k | v] of the new token at position pos (a stopped row, pos < 0: at position 0, where its
    one key is the new one); kc / vc (max_len, D) the row's caches.  Returns the (D,) attention output over [0, pos]."""
    p = max(int(pos), 0)
    D = qkv.shape[0] // 3
    hd = D // H
    c, s = np.asarray(cos[p], F64), np.asarray(sin[p], F64)
    q = rope(np.asarray(qkv[:D], F64).reshape(H, hd), c, s)
    k = rope(np.asarray(qkv[D:2 * D], F64).reshape(H, hd), c, s)
    K = np.asarray(kc[:p + 1], F64).reshape(p + 1, H, hd).copy()
    V = np.asarray(vc[:p + 1], F64).reshape(p + 1, H, hd).copy()
    K[p], V[p] = k, np.asarray(qkv[2 * D:], F64).reshape(H, hd)
    sc = np.einsum("hd,thd->ht", q, K) / np.sqrt(hd)
    pr = np.exp(sc - sc.max(-1, keepdims=True))
    pr /= pr.sum(-1, keepdims=True)
    return np.einsum("ht,thd->hd", pr, V).reshape(D)
