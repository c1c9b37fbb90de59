"""NumPy emulation of the split-fp16 output-resident product (csrc/outres_split.hip) at the contraction the 288 x 288
products give it: K = 288, nine pieces of 32.  tests/test_outres_split_cpu.py holds the emulation and checks K = 768 / 864 /
1536; here the same figure -- worst row of max_d |err| / (max_k |A[t]| max_k |W[d]|) against float64 -- is held to twice
that of an fp32 product summed in pieces of 32, with fp16 subnormals kept and flushed, for the row kinds of that file and for
the special rows of tests/test_rowtile_split_forms_gpu.py (a row scaled by 3e5, one by 1e-7, one element 1e4 above its row,
an all-zero row), with bias and residual added as the kernel adds them: (x + bias) + residual in fp32."""
import numpy as np
import pytest

from tests.test_outres_split_cpu import KINDS, emulate_fp32, emulate_split, figure, make_a, make_w

K = 288
ROWS = 64


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "outlier"])
def test_nine_pieces_within_twice_the_fp32_operands(kind):
    rng = np.random.default_rng(288 + KINDS.index(kind))
    w, a = make_w(K, rng), make_a(kind, ROWS, K, rng)
    fp32 = figure(emulate_fp32(a, w), a, w)
    for flush in (False, True):
        got, moves = emulate_split(a, w, flush)
        split = figure(got, a, w)
        print(f"K {K} {kind:10s} fp32 {fp32:.3e}   split {split:.3e} ({'flushed' if flush else 'kept'})   moves of S {int(moves.max())}")
        assert np.isfinite(got).all() and split <= 2.0 * fp32, (kind, flush, split, fp32)
        if kind == "zero_row":
            assert (got[::3] == 0).all()


def test_late_outlier_is_finite_and_bounded():
    rng = np.random.default_rng(5)
    w, a = make_w(K, rng), make_a("outlier", ROWS, K, rng)
    kept, mk = emulate_split(a, w, False)
    flushed, mf = emulate_split(a, w, True)
    assert np.isfinite(kept).all() and np.isfinite(flushed).all()
    assert (mk == 1).all() and (mf == 1).all()                           # the rescale of the sums ran once in every row
    assert figure(kept, a, w) <= 2.0 * figure(flushed, a, w)


def test_special_rows_with_bias_and_residual():
    rng = np.random.default_rng(9)
    w = make_w(K, rng)
    a = rng.standard_normal((ROWS, K)).astype(np.float32)
    a[3] *= np.float32(3e5)
    a[5] *= np.float32(1e-7)
    a[7, K - 40] *= np.float32(1e4)
    a[9] = 0.0
    bias = rng.standard_normal(288).astype(np.float32)
    res = rng.standard_normal((ROWS, 288)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)[None, :] + res.astype(np.float64)
    fp32 = (emulate_fp32(a, w) + bias[None, :]) + res
    worst = {}
    for flush in (False, True):
        got, _ = emulate_split(a, w, flush)
        out = (got + bias[None, :]) + res
        assert out.dtype == np.float32
        assert np.array_equal(out[9], bias + res[9])                     # an all-zero row: bias + residual exactly
        err = np.abs(out.astype(np.float64) - ref).max(1) / np.abs(ref).max(1)
        worst[flush] = float(err.max())
    base = float((np.abs(fp32.astype(np.float64) - ref).max(1) / np.abs(ref).max(1)).max())
    print(f"worst row error over the row's largest |output|: fp32 {base:.3e}, split {worst[False]:.3e} / {worst[True]:.3e} (kept / flushed)")
    assert worst[False] <= 2.0 * base and worst[True] <= 2.0 * base
