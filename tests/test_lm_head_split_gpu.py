"""The lm_head forward on split-fp16 MFMA (csrc/lm_head_split.hip: pdn_linear_rowmax_split_fwd_f32) against float64 and
against the fp32 MFMA kernel it replaces at 16384 rows and more (pdn_linear_rowmax_fwd_f32, called directly: it is not the
code under test).  `x @ W + b` of pydynet/core/tensor.py:657-676 with the row maxima of nn/functional.py:364-381.

Criterion: the worst row error relative to the row's largest |logit| (float64 reference on sampled rows, the special rows
always among them) of the split kernel is at most 2 x that of the fp32 kernel on the same inputs.  The factor 2 only
allows for a different summation order: the arithmetic is at parity (tests/test_lm_head_split_cpu.py: 1.13e-6 against
1.12e-6 of an fp32 BLAS product).  Measured on an MI355X over the twelve cases: split 3.4e-7 .. 4.3e-7, fp32 kernel
8.3e-7 .. 1.11e-6.

Special rows / columns: a row scaled by 3e5 and one by 1e-7 (both outside fp16's range before scaling), a row with one
1e4 outlier, an all-zero row (its logits are the bias), a column of 1e-6-sized weights, a NaN row (stays NaN)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 288
R_BIG, R_SMALL, R_OUTLIER, R_ZERO, C_TINY = 3, 5, 7, 9, 17


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    import ctypes
    buf = (ctypes.c_int64 * 38)()
    L.call("pdn_kernel_counters", buf, 38, 1 if reset else 0)
    return list(buf)


def _inputs(M, V, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K), dtype=np.float32)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    x[R_BIG] *= np.float32(3e5)
    x[R_SMALL] *= np.float32(1e-7)
    x[R_OUTLIER, 11] = 1e4
    x[R_ZERO] = 0.0
    x[M - 1, 100] = np.nan
    w[:, C_TINY] = (1e-6 * rng.standard_normal(K)).astype(np.float32)
    return x, w, b


def _worst(got, ref):
    """worst over the rows of max |err| / max |logit| (a row of zeros: its error must be zero)."""
    err, scale = np.abs(got.astype(np.float64) - ref).max(1), np.abs(ref).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


@pytest.mark.parametrize("V", [32000, 4000])
@pytest.mark.parametrize("M", [16384, 65536, 65536 + 37])
@pytest.mark.parametrize("bias", [True, False])
def test_split_projection_at_fp32_accuracy(hip, M, V, bias):
    L, hp = _lib_hp()
    assert L.query("pdn_linear_rowmax_split_supported", M, V, K)
    x, w, b = _inputs(M, V, M + V)
    xd, wd, bd = hp.from_numpy(x), hp.from_numpy(w), hp.from_numpy(b)
    bp = bd._ptr if bias else None
    rows = np.unique(np.concatenate([[R_BIG, R_SMALL, R_OUTLIER, R_ZERO, 0, M - 2],
                                     np.random.default_rng(1).integers(0, M - 1, 48)]))
    ref = x[rows].astype(np.float64) @ w.astype(np.float64) + (b.astype(np.float64) if bias else 0.0)

    def split():
        parts = L.query("pdn_linear_rowmax_split_parts", M, V, K)
        assert parts >= 1
        logits, mx = hp.empty((M, V), np.float32), hp.empty((parts, M), np.float32)
        logits[...] = 5.0
        mx[...] = 99.0
        ws, wsb = hp.workspace(L.query("pdn_linear_rowmax_split_workspace_bytes", M, V, K))
        L.call("pdn_linear_rowmax_split_fwd_f32", xd._ptr, wd._ptr, bp, logits._ptr, mx._ptr, M, V, K, K, V, V, ws, wsb, hp.stream())
        return logits, mx.get().max(0)

    _counters(L, True)
    lg, m = split()
    cnt = _counters(L, True)
    assert cnt[5] == 1 and cnt[37] == 1, (cnt[5], cnt[37])
    # the fp32 kernel on the same inputs
    parts32 = L.query("pdn_linear_rowmax_parts", M, V, K)
    lg32, mx32 = hp.empty((M, V), np.float32), hp.empty((parts32, M), np.float32)
    L.call("pdn_linear_rowmax_fwd_f32", xd._ptr, wd._ptr, bp, lg32._ptr, mx32._ptr, M, V, K, K, V, V, hp.stream())
    cnt = _counters(L, True)
    assert cnt[37] == 0

    got = np.stack([lg[int(r)].get() for r in rows])
    got32 = np.stack([lg32[int(r)].get() for r in rows])
    e_split, e_f32 = _worst(got, ref), _worst(got32, ref)
    print(f"M={M} V={V} bias={bias}: worst row error / max |logit|: split {e_split:.3e}, fp32 kernel {e_f32:.3e}")
    assert e_split <= 2.0 * e_f32, f"split-fp16 {e_split:.3e} against 2 x fp32 kernel {e_f32:.3e}"

    # row maxima: bit-equal to the maximum of the logits as stored (every row but the NaN row, the last one)
    stored = lg.max(1).get()
    assert np.array_equal(stored[:M - 1], m[:M - 1])
    # the NaN row stays NaN, the zero row is the bias
    assert np.isnan(lg[M - 1].get()).all()
    assert np.array_equal(lg[R_ZERO].get(), b if bias else np.zeros(V, np.float32))
    # the column of 1e-6-sized weights at ITS OWN scale (without a bias, which would swamp it): the same criterion
    if not bias:
        c, c32 = lg[:, C_TINY:C_TINY + 1].get()[rows, 0], lg32[:, C_TINY:C_TINY + 1].get()[rows, 0]
        keep = rows != R_ZERO
        ec = np.abs(c[keep] - ref[keep, C_TINY]) / np.abs(x[rows[keep]]).max(1)
        ec32 = np.abs(c32[keep] - ref[keep, C_TINY]) / np.abs(x[rows[keep]]).max(1)
        assert ec.max() <= 2.0 * ec32.max(), (ec.max(), ec32.max())

    # a second launch: bit-identical (fixed order, no atomics)
    lg2, m2 = split()
    assert np.array_equal(m2[:M - 1], m[:M - 1])
    assert float((lg[:M - 1] != lg2[:M - 1]).sum().get()) == 0.0
    assert np.isnan(lg2[M - 1].get()).all()


def test_extreme_scales_neither_overflow_nor_underflow(hip):
    """Rows near the ends of fp32's range against columns at the other end: the exponents are integers summed before
    one ldexp, so a finite fp32 result stays finite and a representable one does not vanish."""
    L, hp = _lib_hp()
    M, V = 16384, 128
    rng = np.random.default_rng(5)
    x = rng.standard_normal((M, K), dtype=np.float32)
    w = rng.standard_normal((K, V)).astype(np.float32)
    x[0] *= np.float32(1e30); w[:, 0] *= np.float32(1e-30)          # product of order 1
    x[1] *= np.float32(1e-30); w[:, 1] *= np.float32(1e30)
    x[2] *= np.float32(1e-20); w[:, 2] *= np.float32(1e-20)         # 1e-40: subnormal, not zero
    x[3] *= np.float32(1e18); w[:, 3] *= np.float32(1e18)           # 1e36: close to the top
    xd, wd = hp.from_numpy(x), hp.from_numpy(w)
    parts = L.query("pdn_linear_rowmax_split_parts", M, V, K)
    logits, mx = hp.empty((M, V), np.float32), hp.empty((parts, M), np.float32)
    ws, wsb = hp.workspace(L.query("pdn_linear_rowmax_split_workspace_bytes", M, V, K))
    L.call("pdn_linear_rowmax_split_fwd_f32", xd._ptr, wd._ptr, None, logits._ptr, mx._ptr, M, V, K, K, V, V, ws, wsb, hp.stream())
    parts32 = L.query("pdn_linear_rowmax_parts", M, V, K)
    lg32, mx32 = hp.empty((M, V), np.float32), hp.empty((parts32, M), np.float32)
    L.call("pdn_linear_rowmax_fwd_f32", xd._ptr, wd._ptr, None, lg32._ptr, mx32._ptr, M, V, K, K, V, V, hp.stream())
    got, got32 = logits[:8].get().astype(np.float64), lg32[:8].get().astype(np.float64)
    ref = x[:8].astype(np.float64) @ w.astype(np.float64)
    # (big row x big column overflows in exact arithmetic too: those elements are left out)
    fits = np.abs(ref) < 1e38
    assert np.isfinite(got[fits]).all() and fits[0, 0] and fits[1, 1] and fits[3, 3] and abs(ref[3, 3]) > 1e35
    # results below fp32's normal range: the scaled sum is rounded ONCE onto the subnormal grid (steps of 2^-149), so one
    # step is allowed on top of the criterion of the test above, taken for every ELEMENT at its own scale,
    # max |x_row| max |w_col|
    assert 0 < abs(ref[2, 2]) < 1e-38 and got[2, 2] != 0
    scale = np.abs(x[:8].astype(np.float64)).max(1)[:, None] * np.abs(w.astype(np.float64)).max(0)[None, :]
    step = 2.0 ** -149
    e = (np.maximum(np.abs(got - ref) - step, 0.0) / scale)[fits].max()
    e32 = (np.maximum(np.abs(got32 - ref) - step, 0.0) / scale)[fits].max()
    assert e <= 2.0 * e32, (e, e32)


def test_linear_cross_entropy_with_the_switch_on_and_off(hip):
    """The tape node at 16384 rows: loss and all gradients against float64 and the separate nodes at the 1e-4 criterion
    of tests/test_linear_ce.py, on the split kernel and with it switched off."""
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    from tests.test_linear_ce import _case
    L, _ = _lib_hp()
    saved = (fused.linear_cross_entropy.split_forward, fused.linear_cross_entropy.min_rows)
    try:
        for on in (True, False):
            fused.linear_cross_entropy.split_forward = on
            Graph.clear()
            _counters(L, True)
            _case("hip:0", 16384, 3072, "mean", 0.5, 11)
            cnt = _counters(L, True)
            assert (cnt[37] >= 1) == on and cnt[5] >= 1, (on, cnt[5], cnt[37])
    finally:
        fused.linear_cross_entropy.split_forward, fused.linear_cross_entropy.min_rows = saved
