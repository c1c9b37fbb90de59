"""The lm_head input gradient on split-fp16 MFMA (csrc/lm_head_dx_split.hip: pdn_linear_ce_dx_deferred_split_f32) against
float64 and against the fp32 MFMA kernel it replaces at 32768 rows and more (pdn_linear_ce_dx_deferred_f32, called
directly).  `grad @ W^T` of pydynet/core/tensor.py:670 behind the cross entropy of nn/functional.py:364-381:

    dx[t] = gscale (sum_v e[t][v] W[:, v] / Z[t] - W[:, target[t]]),  e = exp(logit - rowmax),  lse[t] = rowmax[t] + log Z[t]

Logits and row maxima are produced once by pdn_linear_rowmax_fwd_f32 (not code under test) and given to BOTH entries; the
float64 reference is formed from the logits as stored.  Criterion for dx: max |err| / (gscale max |W|) per row -- u / Z is a
convex combination of W's columns, so that is dx's natural scale (the all-probability row's true gradient is ~1e-16: a
row-relative figure would measure nothing there) -- and per output column at gscale max |W[d, :]| (covers the row of
1e-6-sized weights): split <= 2 x the fp32 kernel's figure on the same inputs.  The factor 2 only allows for a different
summation order: the arithmetic is at parity (tests/test_lm_head_dx_split_cpu.py).  lse: float64 at the criterion of
tests/test_fullsize_properties_gpu.py (rtol 1e-6, atol 1e-5); split against fp32 kernel over ALL rows within 2 x the fp32
kernel's worst error on the sampled rows.

Special rows: all probability on the target (row 7: max |dx| < 1e-9 at gscale = 1 / M), a sharp row (x 8), a flat row
(x 0.01), a NaN row (NaN in that row of dx and nowhere else), an out-of-range target (clamped, as in the fp32 kernel)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 288
R_ALL, R_SHARP, R_FLAT, R_BADT, D_TINY = 7, 8, 9, 11, 17


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    import ctypes
    buf = (ctypes.c_int64 * 40)()
    L.call("pdn_kernel_counters", buf, 40, 1 if reset else 0)
    return list(buf)


def _inputs(M, V, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K), dtype=np.float32)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    t = rng.integers(0, V, M).astype(np.int64)
    x[R_ALL] = 40.0 * w[:, t[R_ALL]] / np.linalg.norm(w[:, t[R_ALL]])
    x[R_SHARP] *= np.float32(8.0)
    x[R_FLAT] *= np.float32(0.01)
    x[M - 1, 100] = np.nan
    w[D_TINY, :] *= np.float32(1e-6)
    t[R_BADT] = V + 5
    return x, w, b, t


@pytest.mark.parametrize("V", [32000, 4000])
@pytest.mark.parametrize("M", [57344, 65536, 65536 + 37])
def test_split_input_gradient_at_fp32_accuracy(hip, M, V):
    L, hp = _lib_hp()
    assert L.query("pdn_linear_ce_dx_deferred_split_supported", M, V, K) == 1
    x, w, b, t = _inputs(M, V, M + V)
    xd, wd, bd, td = hp.from_numpy(x), hp.from_numpy(w), hp.from_numpy(b), hp.from_numpy(t)
    parts = L.query("pdn_linear_rowmax_parts", M, V, K)
    logits, mx = hp.empty((M, V), np.float32), hp.empty((parts, M), np.float32)
    L.call("pdn_linear_rowmax_fwd_f32", xd._ptr, wd._ptr, bd._ptr, logits._ptr, mx._ptr, M, V, K, K, V, V, hp.stream())
    gscale = 1.0 / M

    def run(entry):
        dx, lse = hp.empty((M, K), np.float32), hp.empty((M,), np.float32)
        dx[...] = 5.0
        lse[...] = 99.0
        ws, wsb = hp.workspace(L.query(entry.replace("_f32", "_workspace_bytes"), M, V, K))
        L.call(entry, logits._ptr, mx._ptr, parts, td._ptr, gscale, wd._ptr, dx._ptr, lse._ptr, M, V, K, ws, wsb, hp.stream())
        return dx.get(), lse.get()

    _counters(L, True)
    dx_s, lse_s = run("pdn_linear_ce_dx_deferred_split_f32")
    cnt = _counters(L, True)
    assert cnt[12] == 1 and cnt[39] == 1, (cnt[12], cnt[39])
    dx_f, lse_f = run("pdn_linear_ce_dx_deferred_f32")
    cnt = _counters(L, True)
    assert cnt[12] == 1 and cnt[39] == 0, (cnt[12], cnt[39])

    # float64 from the logits as stored, on sampled rows and the special ones
    rows = np.unique(np.concatenate([[R_ALL, R_SHARP, R_FLAT, R_BADT, 0, M - 2],
                                     np.random.default_rng(1).integers(0, M - 1, 50)]))
    lg = np.stack([logits[int(r)].get() for r in rows]).astype(np.float64)
    w64 = w.astype(np.float64)
    m64 = lg.max(1)
    e64 = np.exp(lg - m64[:, None])
    z64 = e64.sum(1)
    tc = np.clip(t[rows], 0, V - 1)
    dx_ref = gscale * ((e64 @ w64.T) / z64[:, None] - w64[:, tc].T)
    lse_ref = m64 + np.log(z64)

    wmax, wmax_d = np.abs(w64).max(), np.abs(w64).max(1)

    def figures(dx):
        err = np.abs(dx[rows].astype(np.float64) - dx_ref)
        return float(err.max() / (gscale * wmax)), float((err.max(0) / (gscale * wmax_d)).max())

    (r_s, c_s), (r_f, c_f) = figures(dx_s), figures(dx_f)
    print(f"M={M} V={V}: dx max |err| / (gscale max |W|): split {r_s:.3e}, fp32 kernel {r_f:.3e}; "
          f"per column at its own scale: split {c_s:.3e}, fp32 kernel {c_f:.3e}")
    assert r_s <= 2.0 * r_f, f"rows: split-fp16 {r_s:.3e} against 2 x fp32 kernel {r_f:.3e}"
    assert c_s <= 2.0 * c_f, f"columns: split-fp16 {c_s:.3e} against 2 x fp32 kernel {c_f:.3e}"

    # lse
    e_s, e_f = np.abs(lse_s[rows] - lse_ref).max(), np.abs(lse_f[rows] - lse_ref).max()
    d_all = np.abs(lse_s[:M - 1].astype(np.float64) - lse_f[:M - 1].astype(np.float64)).max()
    print(f"M={M} V={V}: lse max |err|: split {e_s:.3e}, fp32 kernel {e_f:.3e}; max |split - fp32| over all rows {d_all:.3e}")
    assert np.allclose(lse_s[rows], lse_ref, rtol=1e-6, atol=1e-5)
    assert d_all <= 2.0 * e_f, (d_all, e_f)

    # all probability on the target: the gradient vanishes
    assert np.abs(dx_s[R_ALL]).max() < 1e-9, np.abs(dx_s[R_ALL]).max()
    # the NaN row, and only it
    nan_rows = np.isnan(dx_s).any(1)
    assert np.isnan(dx_s[M - 1]).all() and not nan_rows[:M - 1].any()
    assert np.isnan(lse_s[M - 1]) and not np.isnan(lse_s[:M - 1]).any()
    # the out-of-range target: clamped, as the fp32 kernel does
    assert np.abs(dx_s[R_BADT].astype(np.float64) - dx_f[R_BADT]).max() <= 2.0 * r_f * gscale * wmax + 2.0 * r_s * gscale * wmax

    # a second launch: bit-identical (fixed order, no atomics)
    dx_2, lse_2 = run("pdn_linear_ce_dx_deferred_split_f32")
    assert np.array_equal(dx_2.view(np.uint32)[:M - 1], dx_s.view(np.uint32)[:M - 1])
    assert np.array_equal(lse_2[:M - 1], lse_s[:M - 1]) and np.isnan(dx_2[M - 1]).all()


def test_shapes_the_split_kernel_leaves_to_the_fp32_kernel(hip):
    L, _ = _lib_hp()
    q = lambda M, V, Kin: L.query("pdn_linear_ce_dx_deferred_split_supported", M, V, Kin)
    assert q(131072, 32000, K) == 1 and q(32768, 32000, K) == 1
    assert q(16384, 32000, K) == 0 and q(65536, 32000, 512) == 0 and q(65536, 32016, K) == 0
    assert L.query("pdn_linear_ce_dx_deferred_split_workspace_bytes", 16384, 32000, K) == 0


def test_linear_cross_entropy_with_the_switch_on_and_off(hip):
    """The tape node at 57344 rows: loss and all gradients against float64 and the separate nodes at the 1e-4 criterion
    of tests/test_linear_ce.py, on the split input-gradient kernel and with it switched off."""
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    from tests.test_linear_ce import _case
    L, _ = _lib_hp()
    saved = (fused.linear_cross_entropy.split_dx, fused.linear_cross_entropy.min_rows)
    try:
        for on in (True, False):
            fused.linear_cross_entropy.split_dx = on
            Graph.clear()
            _counters(L, True)
            _case("hip:0", 57344, 3072, "mean", 0.5, 11)
            cnt = _counters(L, True)
            assert (cnt[39] >= 1) == on and cnt[12] >= 1, (on, cnt[12], cnt[39])
    finally:
        fused.linear_cross_entropy.split_dx, fused.linear_cross_entropy.min_rows = saved
