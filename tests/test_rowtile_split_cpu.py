"""The arithmetic of the split-fp16 q | k | v and gate | up projections (csrc/rowtile_split.hip) in NumPy, against float64.

What the kernel does to a row: RMSNorm with the fp32 kernel's arithmetic (x * (1 / r) * w), the row's power of two from
max |x w| * (1 / r) -- NOT from max |xn|, which would need a third sweep over the row; the two differ by round-off, i.e. by
at most one place of the top bit --, two fp16 planes of the scaled xn, three fp16 products with fp32 sums against the
planes of W (one power of two per column), one ldexp with the sum of the two exponents, then RoPE or SwiGLU.
Inputs: 512 rows of width 288 with row scales in [0.2, 3), norm weights in [0.5, 1.5), weights 0.08 N(0, 1) (the ranges of
tests/test_fused_epilogues.py), plus a row scaled by 3e5, one by 1e-7 and one with a single 1e4 outlier.

Asserted, with fp16 subnormals kept AND flushed to zero: the worst row error relative to the row's largest |output| of
q | k | v (rotated), gate | up and h is at most 2 x that of an fp32 BLAS product of the same (fp32-normalised) rows, and
the scaled rows land in [2^7, 2^10) -- the window in which two 11-bit planes still hold 22 bits of the row's largest value."""
import numpy as np
import pytest

K = D = 288
F, ROWS, LQ, HD, EPS = 768, 512, 64, 48, np.float32(1e-6)


def _shift(amax):
    _, e = np.frexp(amax)
    return np.where((amax > 0) & np.isfinite(amax), 9 - e, 0).astype(np.int32)


def _planes(t, ftz):
    h = t.astype(np.float16).astype(np.float32)
    l = ((t - h) * np.float32(2048.0)).astype(np.float16).astype(np.float32)
    if ftz:
        h = np.where(np.abs(h) < 2.0 ** -14, np.float32(0), h)
        l = np.where(np.abs(l) < 2.0 ** -14, np.float32(0), l)
    return h, l


def norm_rows(x, wn, norm):
    """xn, rms and the row exponents as the kernel forms them (float32 throughout)."""
    if not norm:
        return x, None, _shift(np.abs(x).max(1))
    ss = (x * x).sum(1, dtype=np.float32)
    r = np.sqrt(ss / np.float32(288.0) + EPS).astype(np.float32)
    inv = (np.float32(1.0) / r).astype(np.float32)
    xn = (x * inv[:, None]) * wn[None, :]
    amax = np.abs(x * wn[None, :]).max(1) * inv
    return xn.astype(np.float32), r, _shift(amax)


def split_product(xn, sx, w, ftz):
    sw = _shift(np.abs(w).max(0))
    xh, xl = _planes(np.ldexp(xn, sx[:, None]).astype(np.float32), ftz)
    wh, wl = _planes(np.ldexp(w, sw[None, :]).astype(np.float32), ftz)
    acc0 = xh @ wh
    acc1 = xh @ wl + xl @ wh
    return np.ldexp(acc0 + acc1 / np.float32(2048.0), -(sx[:, None] + sw[None, :])).astype(np.float32)


def _rope(y, cos, sin, dt):
    n, C = y.shape
    yh = y.reshape(n, C // HD, HD // 2, 2)
    pos = np.arange(n) % LQ
    c, s = cos[pos][:, None, :].astype(dt), sin[pos][:, None, :].astype(dt)
    out = np.empty_like(yh)
    out[..., 0] = yh[..., 0] * c - yh[..., 1] * s
    out[..., 1] = yh[..., 0] * s + yh[..., 1] * c
    return out.reshape(n, C)


def _silu_mul(g, u):
    return g / (1 + np.exp(-g)) * u


def _worst(got, ref):
    return float((np.abs(got.astype(np.float64) - ref).max(1) / np.abs(ref).max(1)).max())


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(9)
    x = (rng.standard_normal((ROWS, K)) * rng.uniform(0.2, 3.0, (ROWS, 1))).astype(np.float32)
    x[8] *= np.float32(3e5)
    x[9] *= np.float32(1e-7)
    x[10, 11] = 1e4
    wn = rng.uniform(0.5, 1.5, K).astype(np.float32)
    wqkv = (0.08 * rng.standard_normal((K, 3 * D))).astype(np.float32)
    wgu = (0.08 * rng.standard_normal((K, 2 * F))).astype(np.float32)
    inv = 1.0 / (10000 ** (np.arange(0, HD, 2)[: HD // 2] / HD))
    fr = np.outer(np.arange(LQ), inv)
    return x, wn, wqkv, wgu, np.cos(fr).astype(np.float32), np.sin(fr).astype(np.float32)


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("ftz", [False, True])
def test_three_fp16_products_and_the_epilogues_at_fp32_accuracy(data, ftz, norm):
    x, wn, wqkv, wgu, cos, sin = data
    xn, r, sx = norm_rows(x, wn, norm)
    x64 = x.astype(np.float64)
    if norm:
        r64 = np.sqrt((x64 * x64).mean(1) + float(EPS))
        xn64 = x64 / r64[:, None] * wn
        assert np.abs(r - r64).max() <= 2e-6 * np.abs(r64).max() and (np.abs(xn - xn64).max(1) <= 1e-7 + 2e-6 * np.abs(xn64).max(1)).all()
    else:
        xn64 = x64
    top = np.abs(np.ldexp(xn.astype(np.float64), sx[:, None])).max(1)
    assert (top >= 2.0 ** 7).all() and (top < 2.0 ** 10).all()
    # q | k | v + RoPE on q and k
    ref = xn64 @ wqkv.astype(np.float64)
    ref = np.concatenate([_rope(ref[:, :D], cos, sin, np.float64), _rope(ref[:, D:2 * D], cos, sin, np.float64), ref[:, 2 * D:]], 1)

    def rotated(y):
        return np.concatenate([_rope(y[:, :D], cos, sin, np.float32), _rope(y[:, D:2 * D], cos, sin, np.float32), y[:, 2 * D:]], 1)
    e, e32 = _worst(rotated(split_product(xn, sx, wqkv, ftz)), ref), _worst(rotated(xn @ wqkv), ref)
    print(f"norm={norm} ftz={ftz}: worst row error / max |qkv|: fp16 x 3 {e:.3e}, fp32 BLAS {e32:.3e}")
    assert e <= 2.0 * e32, (e, e32)
    # gate | up + SwiGLU
    ref = xn64 @ wgu.astype(np.float64)
    with np.errstate(over="ignore"):
        href = _silu_mul(ref[:, :F], ref[:, F:])
        got, got32 = split_product(xn, sx, wgu, ftz), xn @ wgu
        e, e32 = _worst(got, ref), _worst(got32, ref)
        eh, eh32 = _worst(_silu_mul(got[:, :F], got[:, F:]), href), _worst(_silu_mul(got32[:, :F], got32[:, F:]), href)
    print(f"norm={norm} ftz={ftz}: worst row error / max |gu|: fp16 x 3 {e:.3e}, fp32 BLAS {e32:.3e};  / max |h|: {eh:.3e}, {eh32:.3e}")
    assert e <= 2.0 * e32 and eh <= 2.0 * eh32, (e, e32, eh, eh32)


def test_a_nonfinite_row_keeps_scale_one():
    assert _shift(np.array([np.inf, np.nan, 0.0, 300.0], np.float32)).tolist() == [0, 0, 0, 0]
    assert _shift(np.array([1.0, 3e5, 1e-7], np.float32)).tolist() == [8, -10, 32]
