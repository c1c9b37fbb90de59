"""Float64 statement of what pdn_attention_stream_fwd_f32 / pdn_attention_stream_bwd_f32 compute (include/pdn_hip.h), the
exact statement of the selection pass, and the case builders of tests/test_attention_stream_variants.py.  Plain NumPy on the
logical operands: no tiles, no online softmax, no strides but the ones a case hands to the entry.  Nothing here calls the
package under test.

Operands are (B, L, H, hd) as the entries take them; a mask is broadcastable to (B, H, Lq, Lk)."""
import math
from dataclasses import dataclass

import numpy as np

F32, F64 = np.float32, np.float64
NEG = -np.inf


# =====================================================================================================================
# the statements
# =====================================================================================================================
def rope_tables(n, hd):
    """cos / sin (n, hd / 2) float32, as llm/llama/model.py:23-30 makes them."""
    inv = 1.0 / (10000 ** (np.arange(0, hd, 2) / hd))
    fr = np.outer(np.arange(n), inv).astype(F32)
    return np.cos(fr), np.sin(fr)


def rotate(a, cos, sin, sign):
    """RoPE on (B, L, H, hd) at positions 0 .. L-1 (sign -1: the gradient, the inverse rotation); dtype of `a`."""
    if cos is None:
        return a
    L = a.shape[1]
    c = cos[:L].astype(a.dtype)[None, :, None, :]
    s = (sign * sin[:L]).astype(a.dtype)[None, :, None, :]
    out = np.empty_like(a)
    out[..., 0::2] = a[..., 0::2] * c - a[..., 1::2] * s
    out[..., 1::2] = a[..., 0::2] * s + a[..., 1::2] * c
    return out


def causal_keep(Lq, Lk, causal, start):
    """(Lq, Lk) booleans: the keys a query may see (key <= query + start under the causal flag)."""
    qi, ki = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
    return (ki <= qi + start) if causal else np.ones((Lq, Lk), bool)


def attention(q, k, v, do, causal, start, mask, cos=None, sin=None, dtype=F64):
    """softmax(q k^T / sqrt(hd) + causal + mask) v and its gradients, every operation in `dtype` (float64: the reference;
    float32: the same composition at the kernels' precision, for the peaked rows).  Returns o, lse, dq, dk, dv with
    o, dq (B, Lq, H, hd), lse (B, H, Lq), dk, dv (B, Lk, H, hd)."""
    q, k, v, do = (np.asarray(a, dtype) for a in (q, k, v, do))
    B, Lq, H, hd = q.shape
    Lk = k.shape[1]
    qr, kr = rotate(q, cos, sin, 1.0), rotate(k, cos, sin, 1.0)
    Q, K, V, DO = (a.transpose(0, 2, 1, 3) for a in (qr, kr, v, do))
    scale = dtype(1.0 / math.sqrt(hd))
    s = np.matmul(Q, K.swapaxes(-1, -2)) * scale
    s = s + np.where(causal_keep(Lq, Lk, causal, start), 0.0, NEG).astype(dtype)
    if mask is not None:
        s = s + np.asarray(mask, dtype)
    m = s.max(-1, keepdims=True)
    assert np.isfinite(m).all(), "a fully masked row: not part of this suite"
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = e / l
    o = np.matmul(p, V)
    dv = np.matmul(p.swapaxes(-1, -2), DO)
    dp = np.matmul(DO, V.swapaxes(-1, -2))
    delta = (DO * o).sum(-1, keepdims=True)
    ds = p * (dp - delta) * scale
    dq, dk = np.matmul(ds, K), np.matmul(ds.swapaxes(-1, -2), Q)
    tr = lambda a: a.transpose(0, 2, 1, 3)
    return tr(o), (m + np.log(l))[..., 0], rotate(tr(dq), cos, sin, -1.0), rotate(tr(dk), cos, sin, -1.0), tr(dv)


def selection(pi, v, do):
    """The selection pass: q = 0 and a mask that is 0 at key pi[b, h, q] and -inf (or so low that exp underflows) at every
    other key.  Every score is the mask, p is one-hot, l = 1: o[q] = v[pi(q)], lse = 0, dv[k] = sum of dO[q] over pi(q) = k
    (integers: exact in any order).  With integer v: delta = dP at the selected key, dS = 0, dq = dk = 0."""
    v, do = np.asarray(v, F64), np.asarray(do, F64)
    B, H, Lq = pi.shape
    b, h = np.arange(B)[:, None, None], np.arange(H)[None, :, None]
    o = v[b, pi, h].transpose(0, 2, 1, 3)                              # (B, H, Lq, hd) -> (B, Lq, H, hd)
    dv = np.zeros(v.shape, F64)
    np.add.at(dv, (np.broadcast_to(b, pi.shape), pi, np.broadcast_to(h, pi.shape)), do.transpose(0, 2, 1, 3))
    return o, np.zeros((B, H, Lq), F64), np.zeros(do.shape, F64), np.zeros(v.shape, F64), dv


# =====================================================================================================================
# cases
# =====================================================================================================================
# mask layouts: which of (batch, head, query, key) the mask depends on; "embedded" is a full mask inside a larger buffer
MASK_DIMS = {"BHQK": (1, 1, 1, 1), "11QK": (0, 0, 1, 1), "B11K": (1, 0, 0, 1), "1H1K": (0, 1, 0, 1), "B1QK": (1, 0, 1, 1),
             "1HQ1": (0, 1, 1, 0), "embedded": (1, 1, 1, 1)}


@dataclass
class Case:
    name: str
    B: int
    H: int
    Lq: int
    Lk: int
    hd: int
    causal: int = 0
    start: int = 0
    mask: str = None                 # a key of MASK_DIMS, or None: no mask in the float64 pass
    content: str = "holes"           # "holes": 0 / -inf at random | "normal" | "lead": batch 1 hides its first 40 keys |
    #                                  "trail1e9": -1e9 on trailing keys
    rope: bool = False
    q_mult: int = 1                  # q / o / dO / dq row stride = q_mult * H * hd + q_pad, base q_off * H * hd floats in
    q_off: int = 0
    q_pad: int = 0
    q_gap: int = 0                   # batch stride = (Lq + q_gap) rows
    kv_pad: int = 0
    kv_gap: int = 0                  # k / v / dk / dv batch stride = (Lk + kv_gap) rows: a cache of max_len > Lk
    bs0: bool = False                # B = 1 with both batch strides passed as 0
    qscale: float = 1.0              # 8: the peaked rows
    twice: bool = False              # run the float64 pass twice, bit-equal
    passes: tuple = ("selection", "float64")


@dataclass
class Side:
    """One (B, L, H, hd) operand family in a flat buffer: row / batch strides, base offset, size, all in floats."""
    rs: int
    bs: int
    off: int
    size: int
    shape: tuple

    def logical(self, flat):
        B, L, H, hd = self.shape
        it = flat.itemsize
        return np.lib.stride_tricks.as_strided(flat[self.off:], self.shape, (self.bs * it, self.rs * it, hd * it, it))


def sides(c):
    D = c.H * c.hd
    q_rs, kv_rs = c.q_mult * D + c.q_pad, D + c.kv_pad
    assert c.q_off * D + D <= q_rs and not (c.bs0 and c.B != 1)
    q = Side(q_rs, (c.Lq + c.q_gap) * q_rs, c.q_off * D, c.B * (c.Lq + c.q_gap) * q_rs, (c.B, c.Lq, c.H, c.hd))
    kv = Side(kv_rs, (c.Lk + c.kv_gap) * kv_rs, 0, c.B * (c.Lk + c.kv_gap) * kv_rs, (c.B, c.Lk, c.H, c.hd))
    return q, kv


@dataclass
class MaskLayout:
    """A mask in a flat buffer: compact shape (1 where it broadcasts), element strides (0 where it broadcasts), base offset."""
    shape: tuple
    strides: tuple
    off: int
    size: int

    def logical(self, flat):
        it = flat.itemsize
        st = [s * it for s in self.strides]
        return np.lib.stride_tricks.as_strided(flat[self.off:], self.shape, st)


def mask_layout(kind, B, H, Lq, Lk):
    dims = MASK_DIMS[kind]
    shape = tuple(n if d else 1 for n, d in zip((B, H, Lq, Lk), dims))
    if kind == "embedded":           # key stride 2, query stride 2 Lk + 3, head and batch strides padded, base 4 bytes in
        sk = 2
        sq = 2 * Lk + 3
        sh = Lq * sq + 5
        sb = H * sh + 7
        return MaskLayout(shape, (sb, sh, sq, sk), 1, 1 + B * sb)
    st, acc = [0] * 4, 1
    for i in (3, 2, 1, 0):
        if dims[i]:
            st[i] = acc
            acc *= shape[i]
    return MaskLayout(shape, tuple(st), 0, acc)


def mask_values(c, rng):
    """The float64-pass mask of a case in its compact shape (float32), or None."""
    if c.mask is None:
        return None
    shape = mask_layout(c.mask, c.B, c.H, c.Lq, c.Lk).shape
    if c.content == "normal":
        return rng.standard_normal(shape).astype(F32)
    m = np.zeros(shape, F32)
    if c.content == "holes":
        m[rng.random(shape) < 0.3] = NEG
        m[..., 0] = 0.0                                   # key 0 is admissible for every query: no fully masked row
    elif c.content == "lead":
        assert shape[0] == c.B >= 2 and c.Lk > 40
        m[1, ..., :40] = NEG
    elif c.content == "trail1e9":
        assert shape[0] == c.B
        for b in range(c.B):
            m[b, ..., c.Lk - 10 - 5 * b:] = -1e9
    else:
        raise ValueError(c.content)
    return m


def visible(c, m, zero_only=False):
    """(B, H, Lq, Lk) booleans: keys with a finite mask (zero_only: a mask of exactly 0, what the selection pass may select)
    inside the causal horizon.  Every row keeps one (a condition on the inputs: a fully masked row is NaN in the reference
    too)."""
    keep = np.broadcast_to(causal_keep(c.Lq, c.Lk, c.causal, c.start), (c.B, c.H, c.Lq, c.Lk))
    if m is not None:
        mb = np.broadcast_to(m, keep.shape)
        keep = keep & ((mb == 0.0) if zero_only else np.isfinite(mb))
    assert keep.any(-1).all(), (c.name, "a fully masked row")
    return keep


PI_MODES = ("random", "zero", "diagonal", "last tile")


def choose_pi(c, mode, vis, shape, rng):
    """pi (B, H, Lq): one visible key per query, constant along the dimensions a mask of compact `shape` broadcasts over.
    random | zero: the first visible key (key 0 where it is visible: every query tile accumulates into one dv row) |
    diagonal: the last visible key <= min(Lk - 1, q + start), the last admissible one | last tile: a key of the last 32-key
    tile (non-causal: every earlier tile is fully masked before the first finite score arrives)."""
    full = (c.B, c.H, c.Lq, c.Lk)
    axes = tuple(i for i in range(3) if shape[i] == 1 and full[i] != 1)
    cand = vis.all(axis=axes, keepdims=True) if axes else vis                   # (.., Lk)
    assert cand.any(-1).all(), (c.name, mode, "no key visible to a whole broadcast group")
    keys = np.arange(c.Lk)
    first = cand.argmax(-1)
    last_of = lambda a: c.Lk - 1 - a[..., ::-1].argmax(-1)
    if mode == "random":
        pi = (rng.random(cand.shape) * cand).argmax(-1)
    elif mode == "zero":
        pi = first
    elif mode == "diagonal":
        bound = np.minimum(c.Lk - 1, np.arange(c.Lq) + c.start).reshape(1, 1, c.Lq, 1)
        if cand.shape[2] == 1:
            bound = bound.min(2, keepdims=True)
        under = cand & (keys <= bound)
        pi = np.where(under.any(-1), last_of(under), last_of(cand))
    elif mode == "last tile":
        assert not c.causal
        tail = cand & (keys >= 32 * ((c.Lk - 1) // 32))
        r = (rng.random(cand.shape) * tail).argmax(-1)
        pi = np.where(tail.any(-1), r, last_of(cand))
    else:
        raise ValueError(mode)
    pi = np.broadcast_to(pi, full[:3])
    b, h, q = np.ogrid[:c.B, :c.H, :c.Lq]
    assert vis[b, h, q, pi].all(), (c.name, mode)
    return np.ascontiguousarray(pi)


def selection_mask(pi, shape, Lk, m):
    """The one-hot mask of `pi` in the compact `shape`: 0 at the selected key, elsewhere what the case's own mask holds
    where that is finite and below zero (-1e9: exp underflows to exactly 0), else -inf."""
    idx = tuple(slice(0, n) for n in shape[:3])
    hot = np.arange(Lk) == pi[idx][..., None]
    fill = np.full(shape, NEG, F32)
    if m is not None:
        low = np.isfinite(m) & (m < 0)
        fill[low] = m[low]
    return np.where(hot, F32(0.0), fill).astype(F32)


# ---- the case lists -------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (1, 31, 32, 33, 127, 128, 129, 257)
HEAD_DIMS = (16, 24, 32, 48, 64, 96, 128)
STARTS, START_LQ = (1, 31, 32, 33, 95), (1, 7, 33, 130)


def tile_edge_cases(n):
    """hd 32, Lq = Lk = n on and beside the 32-row tile and the 128-row workgroup, non-causal and causal.

    n = 1, float64 pass, dq and dk: with ONE key p = 1 and dq = dk = 0 in exact arithmetic (the float64 statement gives
    |dq| <= 5e-16), so the criterion 2e-5 max|want| + 1e-7 asks for an absolute error below 1e-7.  The kernels form
    dS = p (dP - delta) / sqrt(hd); with dP = dO . v from the matrix instruction and delta = dO . o summed in another order
    (two float32 sums of magnitude ~ 5 that agree to an ulp or two, times |k| / sqrt(32)) this case measured |dq| = 4.07e-7
    on an MI355X and 2.20e-7 on the emulator, and missed.  The dQ kernel (and the emulator with it) now takes delta from
    the same contraction over the head dim as dP: where a row is one key, o = v and dP - delta is exactly 0."""
    return [Case(f"edge L {n} causal {z}", 1, 2, n, n, 32, causal=z, twice=(n == 257 and z == 1)) for z in (0, 1)]


def unequal_edge_cases():
    """hd 32, non-causal, Lq != Lk across the tile and workgroup edges; and the 513 x 513 anchor at hd 96 (causal, RoPE), the
    only case above 300 positions."""
    return [Case(f"edge Lq {a} Lk {b}", 1, 2, a, b, 32) for a, b in ((33, 129), (129, 33), (1, 300), (160, 31))] + \
        [Case("anchor L 513 hd 96 causal rope", 1, 2, 513, 513, 96, causal=1, rope=True)]


def head_dim_cases(hd):
    """(Lq, Lk) = (129, 161) non-causal and 161 causal: more than one key tile per wave in all three kernels; the partial
    last head-dim tile of 16 / 24 / 48 / 96 with li >= hd % 32.  Random k, v: non-zero in every column."""
    return [Case(f"hd {hd} 129x161", 2, 2, 129, 161, hd), Case(f"hd {hd} 161 causal", 2, 2, 161, 161, hd, causal=1)]


def start_cases(start):
    """Causal with a start position: Lk = start + Lq (the cache), + 40 (keys behind the horizon: dk = dv = 0 exactly),
    - 5 (the horizon clipped by Lk).  hd 48, hd 24 for every third."""
    out = []
    for i, Lq in enumerate(START_LQ):
        for j, extra in enumerate((0, 40, -5)):
            Lk = start + Lq + extra
            if Lk > 0:
                hd = 24 if (3 * i + j + STARTS.index(start)) % 3 == 0 else 48
                out.append(Case(f"start {start} Lq {Lq} Lk {Lk} hd {hd}", 1, 2, Lq, Lk, hd, causal=1, start=start))
    return out


def mask_cases():
    """Every mask layout through the four strides at hd 64, (70, 97), B 2, H 3, and the combinations."""
    kw = dict(B=2, H=3, Lq=70, Lk=97, hd=64)
    out = [Case(f"mask {k}", mask=k, **kw) for k in ("BHQK", "11QK", "B11K", "1H1K", "B1QK", "embedded")]
    out.append(Case("mask 1HQ1 per-(head, query) constant", mask="1HQ1", content="normal", passes=("float64",), **kw))
    out.append(Case("mask BHQK + causal + start 33", mask="BHQK", causal=1, start=33, **kw))
    out.append(Case("mask B11K leading padding", mask="B11K", content="lead", **kw))
    out.append(Case("mask BHQK finite normal", mask="BHQK", content="normal", passes=("float64",), **kw))
    out.append(Case("mask B11K -1e9 trailing", mask="B11K", content="trail1e9", **kw))
    return out


def stride_cases():
    """q / o / dq as a column block of a packed projection; k / v as a slice of a longer cache; B = 1 with batch strides 0;
    both stride sets different in one call (with padded rows on both sides)."""
    kw = dict(H=2, Lq=70, Lk=97, hd=48, causal=1, start=27)
    return [Case("strides: q block of a packed projection", B=2, q_mult=3, q_off=1, **kw),
            Case("strides: k, v slices of a longer cache", B=2, kv_gap=23, **kw),
            Case("strides: B 1, batch strides 0", B=1, bs0=True, **kw),
            Case("strides: both sets differ", B=2, q_mult=3, q_off=1, q_gap=2, kv_gap=23, kv_pad=8, mask="B1QK", **kw)]


def rope_cases():
    """RoPE in the loads (start 0): forward, dq / dk rotated back."""
    return [Case(f"rope L {n} hd {hd}", 2, 2, n, n, hd, causal=int(n == 161), rope=True) for n in (33, 161) for hd in (24, 48, 128)]


def peaked_cases():
    """q scaled by 8: scores of standard deviation about 8, rows dominated by a few keys."""
    return [Case("peaked 161 causal hd 48", 1, 2, 161, 161, 48, causal=1, qscale=8.0, passes=("peaked",)),
            Case("peaked 129x161 hd 64", 2, 1, 129, 161, 64, qscale=8.0, passes=("peaked",))]


def all_cases():
    out = unequal_edge_cases() + mask_cases() + stride_cases() + rope_cases() + peaked_cases()
    for n in EDGE_LENGTHS:
        out += tile_edge_cases(n)
    for hd in HEAD_DIMS:
        out += head_dim_cases(hd)
    for s in STARTS:
        out += start_cases(s)
    return out
