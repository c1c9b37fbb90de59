"""The arithmetic of the split-fp16 lm_head forward (csrc/lm_head_split.hip) in NumPy, against float64.

A product of two fp32 matrices from fp16 operands: every row of x and every column of W is scaled by its own power of two
(largest magnitude into [2^8, 2^9)) and split into a head and a scaled residual, a 2^s = h + l / 2048; the product is
xh wh + (xh wl + xl wh) / 2048 -- fp16 products are exact in fp32, the sums are fp32 -- and the scales leave in one ldexp.
Inputs as in tests/test_fullsize_properties_gpu.py (default_rng(9), x ~ N(0, 1), w ~ 0.05 N(0, 1), K = 288, V = 32000),
512 rows, plus that test's row 7 (one logit takes all the probability), a row scaled by 3e5 and one by 1e-7 (outside
fp16's range before scaling) and a row with a single 1e4 outlier.

What is asserted: the three-product fp16 form, with fp16 subnormals kept AND with them flushed to zero (the kernel must not
depend on what the matrix pipe does with them), meets the row-maxima criterion of the full-size test (rtol 1e-6,
atol 1e-5) and its worst row error, relative to the row's largest |logit|, is at most 2 x that of an fp32 BLAS product
of the same inputs.  The cheaper bf16 form with three products does NOT meet the row-maxima criterion: 8 significand
bits per plane leave 16, not 22."""
import numpy as np
import pytest

K, V, ROWS = 288, 32000, 512


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((ROWS, K), dtype=np.float32)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    t = rng.integers(0, V, ROWS)
    x[7] = 40.0 * w[:, t[7]] / np.linalg.norm(w[:, t[7]])
    x[8] *= np.float32(3e5)
    x[9] *= np.float32(1e-7)
    x[10, 11] = 1e4
    ref = x.astype(np.float64) @ w.astype(np.float64)
    return x, w, ref


def _shift(amax):
    """the exponent that puts amax into [2^8, 2^9); 0 for an all-zero row"""
    _, e = np.frexp(amax)
    return np.where(amax > 0, 9 - e, 0).astype(np.int32)


def _to_bf16(a):
    """round to nearest even onto 8 significand bits, kept in a float32"""
    u = a.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _planes(a, sh, fmt, ftz):
    t = np.ldexp(a, sh).astype(np.float32)
    if fmt == "fp16":
        cast, up = (lambda v: v.astype(np.float16).astype(np.float32)), np.float32(2048.0)
    else:
        cast, up = _to_bf16, np.float32(256.0)
    h = cast(t)
    l = cast((t - h) * up)
    if ftz:                                             # fp16 subnormals (below 2^-14) read as zero
        h = np.where(np.abs(h) < 2.0 ** -14, np.float32(0), h)
        l = np.where(np.abs(l) < 2.0 ** -14, np.float32(0), l)
    return h, l, up


def split_product(x, w, fmt="fp16", ftz=False):
    sx, sw = _shift(np.abs(x).max(1)), _shift(np.abs(w).max(0))
    xh, xl, up = _planes(x, sx[:, None], fmt, ftz)
    wh, wl, _ = _planes(w, sw[None, :], fmt, ftz)
    acc0 = xh @ wh                                      # float32 products of exactly representable factors, float32 sums
    acc1 = xh @ wl + xl @ wh
    return np.ldexp(acc0 + acc1 / up, -(sx[:, None] + sw[None, :])).astype(np.float32)


def _worst_row_error(got, ref):
    return float((np.abs(got.astype(np.float64) - ref).max(1) / np.abs(ref).max(1)).max())


def _maxima_ok(got, ref):
    return np.allclose(got.max(1), ref.max(1), rtol=1e-6, atol=1e-5)


@pytest.mark.parametrize("ftz", [False, True])
def test_three_fp16_products_are_at_fp32_accuracy(data, ftz):
    x, w, ref = data
    got = split_product(x, w, "fp16", ftz)
    e, e32 = _worst_row_error(got, ref), _worst_row_error(x @ w, ref)
    print(f"worst row error / max |logit|: fp16 x 3 (ftz={ftz}) {e:.3e}, fp32 BLAS {e32:.3e}")
    assert _maxima_ok(got, ref)
    assert e <= 2.0 * e32, (e, e32)


def test_fp32_blas_meets_the_row_maxima_criterion(data):
    x, w, ref = data
    assert _maxima_ok(x @ w, ref)


def test_three_bf16_products_are_not(data):
    x, w, ref = data
    got = split_product(x, w, "bf16")
    print(f"worst row error / max |logit|: bf16 x 3 {_worst_row_error(got, ref):.3e}")
    assert not _maxima_ok(got, ref)
    assert not _maxima_ok(got[16:], ref[16:])           # (the plain benchmark-like rows alone)


def test_split_reconstructs_22_bits():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((64, K)).astype(np.float32) * np.float32(3e5)
    sh = _shift(np.abs(a).max(1))
    h, l, up = _planes(a, sh[:, None], "fp16", False)
    t = np.ldexp(a, sh[:, None]).astype(np.float64)
    assert (np.abs(t).max(1) >= 256).all() and (np.abs(t).max(1) < 512).all()
    # head: 11 bits of an element's own magnitude; residual: 11 more, but never finer than fp16's grid at the residual's
    # scale -- relative to the ROW's largest magnitude the reconstruction error stays below 2^-22
    assert (np.abs(h.astype(np.float64) + l.astype(np.float64) / up - t).max(1) <= 2.0 ** -22 * np.abs(t).max(1)).all()
