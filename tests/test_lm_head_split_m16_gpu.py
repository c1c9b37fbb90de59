"""The lm_head forward on `v_mfma_f32_16x16x32_f16` (csrc/lm_head_split.hip: pdn_linear_rowmax_split_fwd_f32, called
directly) at the shapes where its paths differ: few rows, so that the vocabulary is cut into ranges with one tile each
(16384 x 128); rows that are no multiple of 256 with an odd number of 32-column tiles (16384 + 37 x 4000: the guarded
stores, vmcnt(0) waits); and 32768 x 32000 (two ranges of 500 tiles, the steady-state loop with its vmcnt(4) wait).

Reference: float64 on about 64 sampled rows and the special rows -- the first and the last row of a 256-row block, row
M - 1, a row of 1e30 against columns of 1e-30, an all-zero row, a NaN row.  Bounds are those of
tests/test_lm_head_split_gpu.py: the worst row error over the row's largest |logit| is at most 2 x that of the fp32 kernel
(pdn_linear_rowmax_fwd_f32) on the same inputs; row maxima are bit-equal to the maximum of the stored logits, per
vocabulary range; a second launch is bit-identical; the NaN row is NaN and nothing else is; canary values behind row
M - 1 and in the padding of ldl > V are untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 288
R_FIRST, R_LAST, R_BIG, R_ZERO, R_NAN, C_TINY, CANARY = 256, 511, 3, 9, 700, 17, 5.0


def _plan(M, V):
    """ls_plan_tpw / ls_plan_ranges of csrc/lm_head_split_index.h"""
    nt, row_blocks, ns = V // 32, (M + 255) // 256, 1
    while row_blocks * ns < 256 and ns < nt:
        ns += 1
    tpw = (nt + ns - 1) // ns
    return tpw, (nt + tpw - 1) // tpw


def _inputs(M, V, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K), dtype=np.float32)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    x[R_BIG] *= np.float32(1e30)
    w[:, C_TINY] *= np.float32(1e-30)
    x[R_ZERO] = 0.0
    x[R_NAN, 100] = np.nan
    return x, w, b


def _worst(got, ref):
    err, scale = np.abs(got.astype(np.float64) - ref).max(1), np.abs(ref).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


@pytest.mark.parametrize("M,V", [(16384, 128), (16384 + 37, 4000), (32768, 32000)])
def test_forward_on_16x16x32(hip, M, V):
    from pydynet_amd import _lib, hipnp as hp
    L = _lib.lib()
    assert L.query("pdn_linear_rowmax_split_supported", M, V, K)
    tpw, parts = _plan(M, V)
    assert L.query("pdn_linear_rowmax_split_parts", M, V, K) == parts
    x, w, b = _inputs(M, V, M + V)
    xd, wd, bd = hp.from_numpy(x), hp.from_numpy(w), hp.from_numpy(b)
    rows = np.unique(np.concatenate([[R_FIRST, R_LAST, R_BIG, R_ZERO, 0, M - 1], np.random.default_rng(1).integers(0, M, 64)]))
    rows = rows[rows != R_NAN]
    ref = x[rows].astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    ws, wsb = hp.workspace(L.query("pdn_linear_rowmax_split_workspace_bytes", M, V, K))

    def split(ldl):
        logits, mx = hp.empty((M + 8, ldl), np.float32), hp.empty((parts, M), np.float32)
        logits[...] = CANARY
        mx[...] = 99.0
        L.call("pdn_linear_rowmax_split_fwd_f32", xd._ptr, wd._ptr, bd._ptr, logits._ptr, mx._ptr, M, V, K, K, V, ldl, ws, wsb, hp.stream())
        return logits, mx.get()

    lg, mx = split(V)
    lg32, mx32 = hp.empty((M, V), np.float32), hp.empty((L.query("pdn_linear_rowmax_parts", M, V, K), M), np.float32)
    L.call("pdn_linear_rowmax_fwd_f32", xd._ptr, wd._ptr, bd._ptr, lg32._ptr, mx32._ptr, M, V, K, K, V, V, hp.stream())
    got = np.stack([lg[int(r)].get() for r in rows])
    got32 = np.stack([lg32[int(r)].get() for r in rows])
    e_split, e_f32 = _worst(got, ref), _worst(got32, ref)
    print(f"M={M} V={V}: worst row error / max |logit|: split {e_split:.3e}, fp32 kernel {e_f32:.3e}; {parts} ranges of {tpw} tiles")
    assert e_split <= 2.0 * e_f32, f"split-fp16 {e_split:.3e} against 2 x fp32 kernel {e_f32:.3e}"
    # the 1e-30 column at its own scale on the 1e30 row (a product of order 1), and the zero row: exactly the bias
    i_big = int(np.nonzero(rows == R_BIG)[0][0])
    assert abs(got[i_big, C_TINY] - ref[i_big, C_TINY]) <= 2.0 * max(abs(got32[i_big, C_TINY] - ref[i_big, C_TINY]), 2e-6 * abs(ref[i_big, C_TINY]))
    assert np.array_equal(lg[R_ZERO].get(), b)

    # row maxima: bit-equal to the maximum of the logits as stored -- over all columns for every row but the NaN row, per
    # vocabulary range on the sampled rows
    keep = np.arange(M) != R_NAN
    assert np.array_equal(lg[:M].max(1).get()[keep], mx.max(0)[keep])
    for i in range(parts):
        c0, c1 = 32 * tpw * i, min(V, 32 * tpw * (i + 1))
        assert np.array_equal(got[:, c0:c1].max(1), mx[i][rows]), f"range {i}"
    # the NaN row is NaN and nothing else is; the rows behind M - 1 are untouched
    assert np.isnan(lg[R_NAN].get()).all()
    assert float((lg[:M] != lg[:M]).sum().get()) == float(V)
    assert np.array_equal(lg[M:].get(), np.full((8, V), CANARY, np.float32))

    # a second launch, into rows ldl = V + 32 apart: bit-identical; the padding and the rows behind M - 1 untouched
    lg2, mx2 = split(V + 32)
    assert np.array_equal(mx2[:, keep], mx[:, keep])
    out2 = lg2[:, :V]
    assert float((lg[:M] != out2[:M]).sum().get()) == float(V)          # (the NaN row differs from itself)
    assert np.array_equal(np.stack([lg2[int(r)].get()[:V] for r in rows]), got)
    assert np.array_equal(lg2[:, V:].get(), np.full((M + 8, 32), CANARY, np.float32))
    assert np.array_equal(lg2[M:].get(), np.full((8, V + 32), CANARY, np.float32))
