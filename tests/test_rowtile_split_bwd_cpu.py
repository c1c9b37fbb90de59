"""The arithmetic of dh + SwiGLU backward on split-fp16 MFMA (rts_main_kernel<2> of csrc/rowtile_split.hip) in NumPy, against
float64: the emulation of tests/test_rowtile_split_cpu.py (row power of two from max |dy|, two fp16 planes of the scaled
rows, three fp16 products with fp32 sums against the planes of W_down^T with one power of two per dh column, one ldexp) with
the fp32 SwiGLU backward of gemm_rowtile_kernel<., 2> applied: s = sigmoid(g), sl = g s, dsl = sl (1 - s) + s,
dgate = dh u dsl, dup = dh sl.

Inputs: 512 rows of dy (width 288, row scales in [0.2, 3), a row scaled by 3e5, one by 1e-7, one with a single 1e4 outlier, an
all-zero row), W_down 0.08 N(0, 1) with one row (a dh column) at 1e-6, gate and up from N(0, 1.4) with a block of gates at
+-30.  Asserted, with fp16 subnormals kept AND flushed: the worst row error relative to the row's largest |output|, for dgate
and dup each, is at most 2 x that of an fp32 product summed in pieces of 32 (fp32 partial sums of 32 terms, added in fp32) on
the same inputs with the same epilogue; the small column at its own scale likewise.

Measured ratios (emulation / fp32 in pieces of 32), the same with subnormals kept and flushed: dgate 0.94 (3.46e-7 against
3.69e-7), dup 1.16 (3.47e-7 against 2.99e-7); the small column 1.01 (dgate) and 1.87 (dup).  With the one-BLAS-product
summation of tests/test_rowtile_split_cpu.py's `split_product` the dgate ratio reads 2.9: that is the BLAS order over 288 terms
(the plain fp32 BLAS product reads 2.7 too), not the split, so the emulation here sums k-step by k-step as the MFMAs do."""
import numpy as np
import pytest

from tests.test_rowtile_split_cpu import _planes, _shift

K, F, ROWS = 288, 768, 512
R_BIG, R_SMALL, R_OUTLIER, R_ZERO, C_TINY = 8, 9, 10, 11, 17


def split_product(xn, sx, w, ftz):
    """`split_product` of tests/test_rowtile_split_cpu.py with the kernel's order of summation: one MFMA adds the 16 terms of
    a k-step to an fp32 accumulator, 18 k-steps in ascending order (there one fp32 BLAS product sums all 288 terms in an
    order of its own, which costs 1.2e-6 of a row's largest |dh| on these inputs, as the fp32 BLAS product does: 9.9e-7).
    The 16 terms of a k-step are summed in fp32 here, whatever the MFMA does inside."""
    sw = _shift(np.abs(w).max(0))
    xh, xl = _planes(np.ldexp(xn, sx[:, None]).astype(np.float32), ftz)
    wh, wl = _planes(np.ldexp(w, sw[None, :]).astype(np.float32), ftz)
    acc0 = np.zeros((xn.shape[0], w.shape[1]), np.float32)
    acc1 = np.zeros_like(acc0)
    for k in range(0, K, 16):
        s = slice(k, k + 16)
        acc0 += xh[:, s] @ wh[s]
        acc1 += xh[:, s] @ wl[s]
        acc1 += xl[:, s] @ wh[s]
    return np.ldexp(acc0 + acc1 / np.float32(2048.0), -(sx[:, None] + sw[None, :])).astype(np.float32)


def _pieces32(a, w):
    """fp32 product summed in pieces of 32: each piece's 32 terms in fp32, the pieces added in fp32."""
    out = np.zeros((a.shape[0], w.shape[1]), np.float32)
    for k0 in range(0, K, 32):
        p = np.zeros_like(out)
        for k in range(k0, k0 + 32):
            p += a[:, k:k + 1] * w[k:k + 1, :]
        out += p
    return out


def _swiglu_bwd(dh, g, u, dt):
    one = dt(1.0)
    s = one / (one + np.exp(-g.astype(dt)))
    sl = g.astype(dt) * s
    dsl = sl * (one - s) + s
    return (dh.astype(dt) * u.astype(dt) * dsl).astype(dt), (dh.astype(dt) * sl).astype(dt)


def _worst(got, ref):
    err, scale = np.abs(got.astype(np.float64) - ref).max(1), np.abs(ref).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(15)
    dy = (rng.standard_normal((ROWS, K)) * rng.uniform(0.2, 3.0, (ROWS, 1))).astype(np.float32)
    dy[R_BIG] *= np.float32(3e5)
    dy[R_SMALL] *= np.float32(1e-7)
    dy[R_OUTLIER, 11] = 1e4
    dy[R_ZERO] = 0.0
    wd = (0.08 * rng.standard_normal((F, K))).astype(np.float32)
    wd[C_TINY] = (1e-6 * rng.standard_normal(K)).astype(np.float32)
    g = (1.4 * rng.standard_normal((ROWS, F))).astype(np.float32)
    u = (1.4 * rng.standard_normal((ROWS, F))).astype(np.float32)
    g[40:72, 0:64:2] = 30.0
    g[40:72, 1:64:2] = -30.0
    return dy, wd, g, u


@pytest.mark.parametrize("ftz", [False, True])
def test_dh_on_three_fp16_products_and_the_swiglu_backward_at_fp32_accuracy(data, ftz):
    dy, wd, g, u = data
    wt = np.ascontiguousarray(wd.T)                                        # (288 x F): column n = row n of W_down
    sx = _shift(np.abs(dy).max(1))
    dh64 = dy.astype(np.float64) @ wt.astype(np.float64)
    rg, ru = _swiglu_bwd(dh64, g, u, np.float64)
    dh16, dh32 = split_product(dy, sx, wt, ftz), _pieces32(dy, wt)
    with np.errstate(over="ignore"):
        (g16, u16), (g32, u32) = _swiglu_bwd(dh16, g, u, np.float32), _swiglu_bwd(dh32, g, u, np.float32)
    for name, a, b, ref in (("dgate", g16, g32, rg), ("dup", u16, u32, ru)):
        e, e32 = _worst(a, ref), _worst(b, ref)
        print(f"ftz={ftz}: worst row error / max |{name}|: fp16 x 3 {e:.3e}, fp32 in pieces of 32 {e32:.3e}, ratio {e / e32:.2f}")
        assert e <= 2.0 * e32, (name, e, e32)
    rows = np.array([r for r in range(ROWS) if r != R_ZERO])
    amax = np.abs(dy[rows].astype(np.float64)).max(1)
    for name, a, b, ref in (("dgate", g16, g32, rg), ("dup", u16, u32, ru)):
        fac = np.abs(ref[rows, C_TINY] / dh64[rows, C_TINY])
        ok = fac > 0
        ec = (np.abs(a[rows, C_TINY] - ref[rows, C_TINY])[ok] / (amax[ok] * fac[ok])).max()
        ec32 = (np.abs(b[rows, C_TINY] - ref[rows, C_TINY])[ok] / (amax[ok] * fac[ok])).max()
        print(f"ftz={ftz}: small-weight column of {name}: fp16 x 3 {ec:.3e}, fp32 in pieces of 32 {ec32:.3e}, ratio {ec / ec32:.2f}")
        assert ec <= 2.0 * ec32, (name, ec, ec32)
    assert not g16[R_ZERO].any() and not u16[R_ZERO].any()
