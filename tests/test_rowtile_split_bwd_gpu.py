"""dh + SwiGLU backward on split-fp16 MFMA (rts_main_kernel<2> of csrc/rowtile_split.hip: the form `pdn_swiglu_bwd_gemm_f32`
takes at 16384 rows and more) against float64 and against the fp32 MFMA kernel it replaces there (the same entry under
`pdn_gemm_rowtile_mode(3)`).  dgu = SwiGLU'(gu) o (dy W_down^T): llm/llama/model.py:56-58 backwards.

Criterion (the one of tests/test_rowtile_split_gpu.py): the worst row error relative to the row's largest |output| -- float64
reference on about 65 rows: the special rows, the first and last rows of workgroups, the last row before M, and random ones --
of the split kernel is at most 2 x that of the fp32 kernel on the same inputs, for dgate and dup each; the dh column with
1e-6-sized weights at its own scale.  The SwiGLU backward itself is the same fp32 arithmetic in both kernels, so only dh differs.

Shapes: (M, F) = (16384, 768): four grid.y ranges; (16384 + 37, 768): GUARD; (16384, 192): three ranges of two tiles;
(65536, 96): one range.  dy has a leading dimension of K + 8 with a canary in the padding; gu and dgu carry eight canary rows
behind M.

Special rows: scaled by 3e5 and by 1e-7, one 1e4 outlier, an all-zero row (dgu zero), a NaN row (that row NaN, no other), a
block of gates at +-30 (the sigmoid saturates).  An in-place call (dgu over gu) never takes the split form (gemm_rowres.hip
sends it to the chunk kernel): it equals the out-of-place result of the fp32 kernels bit for bit -- the split form's result
differs from both in the last bits, so that is the out-of-place result it can be held to -- and leaves slot 51 at 0.

Measured on an MI355X over the four cases (every case prints its figures; profiles/rowtile_split_bwd_gpu_tests.txt): dgate
split 3.1e-7 .. 4.3e-7 against the fp32 kernel's 7.3e-7 .. 1.07e-6; dup 3.1e-7 .. 4.0e-7 against 6.8e-7 .. 9.2e-7; the
small-weight column 0.50 .. 1.07 x the fp32 kernel's figure.  One training step (2 layers, 16384 tokens): the loss agrees to
all printed digits (5.2128386), gradients within 3.8e-6 of their largest entry."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 288
R_BIG, R_SMALL, R_OUTLIER, R_ZERO, R_NAN, C_TINY = 3, 5, 7, 9, 11, 17
SAT0, SAT1 = 40, 72                                   # rows whose first 64 gates are +-30
CANARY = np.float32(7.5)
PAD = 8
SLOTS = 52


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    buf = (ctypes.c_int64 * SLOTS)()
    L.call("pdn_kernel_counters", buf, SLOTS, 1 if reset else 0)
    return list(buf)


def _rows(M):
    fixed = [R_BIG, R_SMALL, R_OUTLIER, R_ZERO, R_NAN, 0, 31, 32, 255, 256, 511, SAT0, SAT1 - 1, M - 257, M - 256, M - 2, M - 1]
    return np.unique(np.concatenate([fixed, np.random.default_rng(1).integers(0, M, 48)]))


def _dy(M, rng):
    dy = np.full((M, K + PAD), 1e30, np.float32)
    dy[:, :K] = rng.standard_normal((M, K), dtype=np.float32)
    dy[R_BIG, :K] *= np.float32(3e5)
    dy[R_SMALL, :K] *= np.float32(1e-7)
    dy[R_OUTLIER, 11] = 1e4
    dy[R_ZERO, :K] = 0.0
    dy[R_NAN, 100] = np.nan
    return dy


def _worst(got, ref):
    """worst over the rows of max |err| / max |output| (a row of zeros: its error must be zero)."""
    err, scale = np.abs(got.astype(np.float64) - ref).max(1), np.abs(ref).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


def _take(arr, rows):
    return np.stack([arr[int(r)].get() for r in rows])


def _inputs(M, F):
    """dy, W_down, and gu from a real forward call with the saturated block put in; everything on the device and on the host."""
    L, hp = _lib_hp()
    rng = np.random.default_rng(M + F)
    dy = _dy(M, rng)
    wd = (0.08 * rng.standard_normal((F, K))).astype(np.float32)
    wd[C_TINY] = (1e-6 * rng.standard_normal(K)).astype(np.float32)
    x = hp.from_numpy(rng.standard_normal((M, K), dtype=np.float32))
    wgu = hp.from_numpy((0.08 * rng.standard_normal((2, K, F))).astype(np.float32))
    gu_d, h = hp.empty((M, 2 * F), np.float32), hp.empty((M, F), np.float32)
    L.call("pdn_gateup_swiglu_fwd_f32", x._ptr, wgu._ptr, K * F, gu_d._ptr, h._ptr, M, F, K, K, hp.stream())
    gu = np.full((M + 8, 2 * F), CANARY, np.float32)
    gu[:M] = gu_d.get()
    gu[SAT0:SAT1, 0:64:2] = 30.0
    gu[SAT0:SAT1, 1:64:2] = -30.0
    return dy, wd, gu


def _ref64(dy, wd, gu, rows, F):
    dh = dy[rows, :K].astype(np.float64) @ wd.astype(np.float64).T
    g, u = gu[rows, :F].astype(np.float64), gu[rows, F:].astype(np.float64)
    s = 1.0 / (1.0 + np.exp(-g))
    return dh, dh * u * s * (1.0 + g * (1.0 - s)), dh * g * s


@pytest.mark.parametrize("M,F", [(16384, 768), (16384 + 37, 768), (16384, 192), (65536, 96)])
def test_swiglu_backward_at_fp32_accuracy(hip, M, F):
    L, hp = _lib_hp()
    dy, wd, gu = _inputs(M, F)
    dyd, wdd, gud = hp.from_numpy(dy), hp.from_numpy(wd), hp.from_numpy(gu)
    rows = _rows(M)
    with np.errstate(invalid="ignore"):
        dh64, dg64, du64 = _ref64(dy, wd, gu, rows, F)

    def run():
        dgu = hp.empty((M + 8, 2 * F), np.float32)
        dgu[...] = CANARY
        L.call("pdn_swiglu_bwd_gemm_f32", dyd._ptr, wdd._ptr, gud._ptr, dgu._ptr, M, F, K, K + PAD, hp.stream())
        return dgu

    _counters(L, True)
    dgu = run()
    cnt = _counters(L, True)
    assert cnt[51] == 1 and cnt[3] == 1 and cnt[41] == 0, (cnt[3], cnt[41], cnt[51])
    prev = L.query("pdn_gemm_rowtile_mode", 3)
    try:
        dgu32 = run()
    finally:
        L.query("pdn_gemm_rowtile_mode", prev)
    cnt = _counters(L, True)
    assert cnt[51] == 0 and cnt[3] == 1, (cnt[3], cnt[51])

    keep = rows != R_NAN
    got, got32 = _take(dgu, rows), _take(dgu32, rows)
    for name, sl, ref in (("dgate", slice(0, F), dg64), ("dup", slice(F, 2 * F), du64)):
        e_split, e_f32 = _worst(got[keep][:, sl], ref[keep]), _worst(got32[keep][:, sl], ref[keep])
        print(f"dh + SwiGLU backward M={M} F={F}: worst row error / max |{name}|: split {e_split:.3e}, fp32 kernel {e_f32:.3e}")
        assert e_split <= 2.0 * e_f32, f"{name}: split-fp16 {e_split:.3e} against 2 x fp32 kernel {e_f32:.3e}"
    # the dh column of 1e-6-sized weights at ITS OWN scale (the row's largest |dy| times the factor SwiGLU' puts on it): the same criterion
    sel = keep & (rows != R_ZERO)
    amax = np.abs(dy[rows[sel], :K].astype(np.float64)).max(1)
    for name, col, ref in (("dgate", C_TINY, dg64), ("dup", F + C_TINY, du64)):
        fac = np.abs(ref[sel, C_TINY] / dh64[sel, C_TINY])
        ok = fac > 0
        ec = np.abs(got[sel][:, col] - ref[sel, C_TINY])[ok] / (amax[ok] * fac[ok])
        ec32 = np.abs(got32[sel][:, col] - ref[sel, C_TINY])[ok] / (amax[ok] * fac[ok])
        print(f"dh + SwiGLU backward M={M} F={F}: small-weight column of {name}: split {ec.max():.3e}, fp32 kernel {ec32.max():.3e}")
        assert ec.max() <= 2.0 * ec32.max(), (name, ec.max(), ec32.max())
    # the NaN row is NaN and no other row is; the zero row is zero; nothing behind M
    assert np.isnan(dgu[R_NAN].get()).all()
    assert np.isfinite(got[keep]).all() and np.isfinite(dgu[R_NAN - 1].get()).all() and np.isfinite(dgu[R_NAN + 1].get()).all()
    assert not dgu[R_ZERO].get().any()
    assert (dgu[M:].get() == CANARY).all()
    assert float(np.abs(got[keep & (rows != R_BIG)]).max()) < 1e20          # (x's padding canary reached nothing)
    # a second launch: bit-identical (fixed order, no atomics)
    dgu2 = run()
    a, b = dgu.get(), dgu2.get()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_in_place_call_stays_on_the_fp32_path(hip):
    L, hp = _lib_hp()
    M, F = 16384, 768
    dy, wd, gu = _inputs(M, F)
    dy[R_NAN, 100] = 0.5                              # (bit comparison below: no NaN)
    dyd, wdd = hp.from_numpy(dy), hp.from_numpy(wd)
    gud, out = hp.from_numpy(gu), hp.empty((M + 8, 2 * F), np.float32)
    out[...] = CANARY
    prev = L.query("pdn_gemm_rowtile_mode", 3)
    try:
        L.call("pdn_swiglu_bwd_gemm_f32", dyd._ptr, wdd._ptr, gud._ptr, out._ptr, M, F, K, K + PAD, hp.stream())
    finally:
        L.query("pdn_gemm_rowtile_mode", prev)
    inplace = hp.from_numpy(gu)
    _counters(L, True)
    L.call("pdn_swiglu_bwd_gemm_f32", dyd._ptr, wdd._ptr, inplace._ptr, inplace._ptr, M, F, K, K + PAD, hp.stream())
    cnt = _counters(L, True)
    assert cnt[51] == 0 and cnt[41] == 0, (cnt[41], cnt[51])
    assert np.array_equal(out.get().view(np.uint32), inplace.get().view(np.uint32))


def test_training_step_with_the_route_on_and_off(hip, monkeypatch):
    import tests.test_rowtile_split_gpu as base
    from tests.test_fused_epilogues import RT
    monkeypatch.setattr(base, "_counters", _counters)                       # the model and step of `_step`, 52 counter slots
    L, _ = _lib_hp()
    l1, g1, c1 = base._step("hip:0", L, 1)
    l0, g0, c0 = base._step("hip:0", L, 3)
    assert c1[51] == 2 and c1[41] == 4 and c1[3] == 2, (c1[3], c1[41], c1[51])
    assert c0[51] == 0 and c0[41] == 0 and c0[3] == 2, (c0[3], c0[41], c0[51])
    print(f"step: loss with the route on {l1:.7f}, fp32 kernels {l0:.7f}")
    assert abs(l1 - l0) <= RT * abs(l0), (l1, l0)
    assert g1.keys() == g0.keys() and len(g1) >= 20
    worst = 0.0
    for n in g0:
        scale = float(np.abs(g0[n]).max())
        err = float(np.abs(g1[n].astype(np.float64) - g0[n]).max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= 1e-4 * scale, (n, err, scale)
    print(f"step: worst gradient difference / largest entry {worst:.3e}")
