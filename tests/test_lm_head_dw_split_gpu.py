"""The lm_head weight gradient on split-fp16 MFMA (csrc/lm_head_dw_split.hip) against float64 and against the fp32 MFMA kernel
it replaces from 32768 rows up (gemm_outres_tn_kernel<.., CE>).  Both run through pdn_linear_ce_backward_f32 with dx = NULL:
the split form when the workspace holds its extra region (counter slot 40 == 1, slot 13 == 1), the fp32 kernel when the
workspace is the fp32 kernels' size (slot 40 == 0, slot 13 == 1) -- the in-process A/B switch of include/pdn_hip.h.

    dW[d][v] = sc sum_t x[t][d] g[t][v],  dbias[v] = sc sum_t g[t][v],  g = exp(logit - lse[t]) - [v == target[t]],
    sc = gscale * upstream

Logits come once from pdn_linear_rowmax_fwd_f32 and lse from pdn_linear_ce_dx_deferred_f32 (neither is code under test) and
are given to BOTH paths; the float64 reference is formed from `logits[:, cols]` and the lse as stored, on ~64 sampled
columns plus column 5 (the target of every 7th token), column V - 1 and a column no token targets.
Figure for dW: max_v |err| / (sc max_t |x[t, d]|) per row d, then the max over d (covers d = 17, the column of x scaled by
1e-6), over the ordinary columns and over the hot column 5 separately; for dbias: max |err| / sc over the same two sets.
Criterion: split <= 2 x the fp32 kernel's figure on the same inputs, for each.  The factor 2 allows for a different
summation order inside a K range; the arithmetic is at parity at equal range counts (tests/test_lm_head_dw_split_cpu.py:
<= 1.31 x), and the split kernel takes the fp32 kernel's ranges.

Shapes: V = 4000 gives 16 K ranges and a last workgroup with idle waves (4000 = 31 x 128 + 32), 32768 + 160 rows an odd
piece count and so unequal ranges, V = 32000 the benchmark's two ranges at the fewest rows."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 288
R_ALL, R_SHARP, R_FLAT, R_BADT, D_TINY, HOT = 7, 8, 9, 11, 17, 5
UPSTREAM = 0.5


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    buf = (ctypes.c_int64 * 41)()
    L.call("pdn_kernel_counters", buf, 41, 1 if reset else 0)
    return list(buf)


def _extra(rows):
    return (rows // 32) * 37888 + 1152                    # the closed formula of include/pdn_hip.h


def _inputs(M, V, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, K), dtype=np.float32)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    t = rng.integers(0, V, M).astype(np.int64)
    t[::7] = HOT
    x[R_ALL] = 40.0 * w[:, t[R_ALL]] / np.linalg.norm(w[:, t[R_ALL]])
    x[R_SHARP] *= np.float32(8.0)
    x[R_FLAT] *= np.float32(0.01)
    x[:, D_TINY] *= np.float32(1e-6)
    t[R_BADT] = V + 5
    return x, w, b, t


class _Problem:
    """logits and lse of one shape, from entries that are not under test; both paths of the backward entry"""

    def __init__(self, M, V, seed):
        L, hp = _lib_hp()
        self.L, self.hp, self.M, self.V = L, hp, M, V
        self.x, self.w, self.b, self.t = _inputs(M, V, seed)
        self.xd, self.wd, self.td = hp.from_numpy(self.x), hp.from_numpy(self.w), hp.from_numpy(self.t)
        bd = hp.from_numpy(self.b)
        parts = L.query("pdn_linear_rowmax_parts", M, V, K)
        self.logits, mx = hp.empty((M, V), np.float32), hp.empty((parts, M), np.float32)
        L.call("pdn_linear_rowmax_fwd_f32", self.xd._ptr, self.wd._ptr, bd._ptr, self.logits._ptr, mx._ptr, M, V, K, K, V, V, hp.stream())
        if L.query("pdn_linear_ce_dx_deferred_supported", M, V, K) == 1:
            dx, self.lse = hp.empty((M, K), np.float32), hp.empty((M,), np.float32)
            ws, wsb = hp.workspace(L.query("pdn_linear_ce_dx_deferred_workspace_bytes", M, V, K))
            L.call("pdn_linear_ce_dx_deferred_f32", self.logits._ptr, mx._ptr, parts, self.td._ptr, 1.0 / M, self.wd._ptr, dx._ptr,
                   self.lse._ptr, M, V, K, ws, wsb, hp.stream())
        else:                                             # (the small shapes of the dispatch test)
            l64 = self.logits.get().astype(np.float64)
            m = l64.max(1)
            self.lse = hp.from_numpy((m + np.log(np.exp(l64 - m[:, None]).sum(1))).astype(np.float32))
        self.up = hp.from_numpy(np.array([UPSTREAM], np.float32))
        self.gscale = 1.0 / M
        self.need = L.query("pdn_linear_ce_workspace_bytes", M, V, K)

    def run(self, split, x=None, dw_beta=0.0, db_beta=0.0, prefill=None):
        """dW, dbias and the counters (slot 13, slot 40) of one call"""
        L, hp, M, V = self.L, self.hp, self.M, self.V
        dw, db = hp.empty((K, V), np.float32), hp.empty((V,), np.float32)
        dw[...] = 5.0 if prefill is None else prefill[0]
        db[...] = 5.0 if prefill is None else prefill[1]
        ws, _ = hp.workspace(self.need)
        wsb = self.need if split else self.need - _extra(M)
        xd = self.xd if x is None else x
        _counters(L, True)
        L.call("pdn_linear_ce_backward_f32", xd._ptr, K, self.logits._ptr, self.lse._ptr, self.td._ptr, self.gscale, self.up._ptr,
               self.wd._ptr, None, None, dw._ptr, dw_beta, db._ptr, db_beta, M, V, K, ws, wsb, hp.stream())
        cnt = _counters(L, True)
        return dw.get(), db.get(), (cnt[13], cnt[40])


@pytest.mark.parametrize("M,V", [(32768, 4000), (32768 + 160, 4000), (32768, 32000)])
def test_split_weight_gradient_at_fp32_accuracy(hip, M, V):
    p = _Problem(M, V, M + V)
    dw_s, db_s, cnt = p.run(True)
    assert cnt == (1, 1), cnt
    dw_f, db_f, cnt = p.run(False)
    assert cnt == (1, 0), cnt

    # float64 from the logits and the lse as stored, on sampled columns and the special ones
    never = int(np.setdiff1d(np.arange(V), p.t)[0])
    cols = np.unique(np.concatenate([[HOT, V - 1, never], np.random.default_rng(1).integers(0, V, 64)]))
    lg = np.concatenate([p.logits[:, int(c):int(c) + 1].get() for c in cols], axis=1).astype(np.float64)
    g = np.exp(lg - p.lse.get().astype(np.float64)[:, None])
    g[p.t[:, None] == cols[None, :]] -= 1.0              # (the out-of-range target matches no column)
    sc = p.gscale * UPSTREAM
    x64 = p.x.astype(np.float64)
    dw_ref, db_ref = sc * (x64.T @ g), sc * g.sum(0)
    xmax = np.abs(x64).max(0)
    hot = cols == HOT

    def figures(dw, db):
        e = np.abs(dw[:, cols].astype(np.float64) - dw_ref) / (sc * xmax[:, None])
        eb = np.abs(db[cols].astype(np.float64) - db_ref) / sc
        return float(e[:, ~hot].max()), float(e[:, hot].max()), float(eb[~hot].max()), float(eb[hot].max())

    fs, ff = figures(dw_s, db_s), figures(dw_f, db_f)
    for name, s, f in zip(("dW, ordinary columns", "dW, hot column", "dbias, ordinary columns", "dbias, hot column"), fs, ff):
        print(f"M={M} V={V}: {name}: split {s:.3e}, fp32 kernel {f:.3e}")
    for name, s, f in zip(("dW, ordinary columns", "dW, hot column", "dbias, ordinary columns", "dbias, hot column"), fs, ff):
        assert s <= 2.0 * f, f"{name}: split-fp16 {s:.3e} against 2 x fp32 kernel {f:.3e}"

    # the whole matrix: no column beyond the sampled ones is off.  |split - fp32| <= the two errors; their maxima over all V
    # columns instead of ~67 are larger by sqrt(ln(288 V) / ln(288 x 67)) < 1.3 for errors that add up like these: 2 x
    d_all = np.abs(dw_s.astype(np.float64) - dw_f) / (sc * xmax[:, None])
    assert d_all.max() <= 2.0 * (max(fs[0], fs[1]) + max(ff[0], ff[1])), d_all.max()
    assert np.isfinite(dw_s).all() and np.isfinite(db_s).all()
    # the out-of-range target: no column is its target, as in the fp32 kernel -- row R_BADT enters every column as p alone;
    # a kernel that clamped it to V - 1 would be off by sc |x| there: V - 1 is among the sampled columns above, and here
    bad = np.abs(dw_s[:, V - 1].astype(np.float64) - dw_f[:, V - 1]).max()
    assert bad <= 0.01 * sc * np.abs(p.x[R_BADT]).max(), bad

    # a second launch: bit-identical (fixed order, no atomics)
    dw_2, db_2, _ = p.run(True)
    assert np.array_equal(dw_2.view(np.uint32), dw_s.view(np.uint32)) and np.array_equal(db_2.view(np.uint32), db_s.view(np.uint32))

    # dw_beta = db_beta = 1 into prefilled outputs: prefill + gradient, rounded at the prefill's magnitude (two units in the
    # last place of 0.25 and of 0.5 + |dbias| < 1: the reduction adds the slabs and the old value in an order of its own)
    dw_b, db_b, cnt = p.run(True, dw_beta=1.0, db_beta=1.0, prefill=(0.25, -0.5))
    assert cnt == (1, 1)
    assert np.abs((dw_b.astype(np.float64) - 0.25) - dw_s).max() <= 2.0 ** -24, np.abs((dw_b.astype(np.float64) - 0.25) - dw_s).max()
    assert np.abs((db_b.astype(np.float64) + 0.5) - db_s).max() <= 2.0 ** -23, np.abs((db_b.astype(np.float64) + 0.5) - db_s).max()


def test_nan_in_x_marks_the_same_entries(hip):
    """one NaN in x (the logits and lse are those of the clean x): row d of dW is NaN and nothing else, in both kernels"""
    M, V = 32768, 256
    p = _Problem(M, V, 3)
    xn = p.x.copy()
    xn[12345, 100] = np.nan
    xd = p.hp.from_numpy(xn)
    dw_s, db_s, cnt = p.run(True, x=xd)
    assert cnt == (1, 1), cnt
    dw_f, db_f, cnt = p.run(False, x=xd)
    assert cnt == (1, 0), cnt
    assert np.array_equal(np.isnan(dw_s), np.isnan(dw_f))
    assert np.isnan(dw_s[100]).all() and not np.isnan(np.delete(dw_s, 100, axis=0)).any()
    assert not np.isnan(db_s).any() and not np.isnan(db_f).any()


def test_shapes_and_workspaces_the_split_kernel_leaves_to_the_fp32_kernel(hip):
    L, hp = _lib_hp()
    # below the row threshold and below the column threshold: the fp32 kernel, whatever the workspace
    for M, V, seed in ((16384, 4000, 5), (32768, 96, 7)):
        p = _Problem(M, V, seed)
        _, _, cnt = p.run(True)
        assert cnt == (1, 0), (M, V, cnt)
    # a supported shape: the full size takes the split kernel, one byte less the fp32 kernel (the size less the whole extra
    # region is asserted for every shape of the accuracy test above)
    M, V = 32768, 256
    p = _Problem(M, V, 6)
    dw = hp.empty((K, V), np.float32)
    ws, _ = hp.workspace(p.need)
    for wsb, want in ((p.need, (1, 1)), (p.need - 1, (1, 0))):
        _counters(L, True)
        L.call("pdn_linear_ce_backward_f32", p.xd._ptr, K, p.logits._ptr, p.lse._ptr, p.td._ptr, p.gscale, None, p.wd._ptr, None, None,
               dw._ptr, 0.0, None, 0.0, M, V, K, ws, wsb, hp.stream())
        cnt = _counters(L, True)
        assert (cnt[13], cnt[40]) == want, (wsb, cnt[13], cnt[40])


def test_linear_cross_entropy_with_the_switch_on_and_off(hip):
    """The tape node at 57344 rows: loss and all gradients against float64 and the separate nodes at the 1e-4 criterion
    of tests/test_linear_ce.py, on the split weight-gradient kernel and with it switched off."""
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    from tests.test_linear_ce import _case
    L, _ = _lib_hp()
    saved = (fused.linear_cross_entropy.split_dw, fused.linear_cross_entropy.min_rows)
    try:
        for on in (True, False):
            fused.linear_cross_entropy.split_dw = on
            Graph.clear()
            _counters(L, True)
            _case("hip:0", 57344, 3072, "mean", 0.5, 11)
            cnt = _counters(L, True)
            assert (cnt[40] >= 1) == on and cnt[13] >= 1, (on, cnt[13], cnt[40])
    finally:
        fused.linear_cross_entropy.split_dw, fused.linear_cross_entropy.min_rows = saved
