"""pdng_outres_blocks_nt_rmsnorm_bwd_f32 (include/pdn_normgrad.h): the layer input gradient with the RMSNorm backward in the
drain of the split-fp16 output-resident kernel (ors_main_kernel<0, 1> of csrc/outres_split.hip) against float64 of its
statement -- pdn_gemm_outres_blocks_nt_f32 with no residual, then pdn_rmsnorm_bwd_f32 on its output -- and against those two
launches themselves on the same inputs.

Shapes, the smallest the split kernel takes: 65536 rows (two full 128-row blocks for each of the 256 workgroups) against 3
blocks of 288; 65536 + 3 x 128 + 5 rows (a ragged walk: some workgroups own a third block, the last block is partial)
against 2 blocks of 768 at falling addresses; the same ragged rows against one block of 256, the shortest K taken.
Inputs: a standard normal gradient with all-zero rows (the first, one in the middle, the last); x standard normal, or its
rows scaled log-uniformly over 1e-3 .. 1e3 (rms with them); with and without dx_residual; dw null, `=` and `+=` (onto a
random vector).
Reference, float64: dx on about 96 rows (sample_rows: twelve rows of each of the eight waves, spread over the first block, two
blocks in between and the last whole block, plus the rows of the last group of a partial last block; the first test checks
that spread) -- and dw over ALL rows (every shape: one per K).
Bound: fused error over the reference's largest entry <= 2 x the same figure of the two launches on the same inputs + 1e-7,
for dx and for dw.  Every case prints both figures; the printout of a run is profiles/norm_bwd_fused_gpu_tests.txt.
Two calls give identical bits; rows >= M of dx keep a canary.
Routes: the launch counter of the fused kernel reads 1 per call on the split route and 0 with PDN_NORM_BWD_FUSE=0, where dx
and dw equal the two launches bit for bit.  Below 65536 rows it reads 0 as well: at 57344 rows (the fewest at which
pdn_gemm_outres_blocks_nt_f32 answers, so the two launches can be called) the results equal theirs bit for bit; at 4096 rows,
where that entry declines, the two launches cannot be called from outside: the entry is compared with itself under the
switch, which is TRIVIALLY true there (both calls take the two-launch route) and only shows that the switch changes nothing;
what the 4096-row case asserts is the counter and float64 at fp32 accuracy."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 288
MMIN = 65536
CANARY = np.float32(7.5)
ENTRY = "pdng_outres_blocks_nt_rmsnorm_bwd_f32"
# (M, kb, nb, falling addresses)
SHAPES = [(MMIN, 288, 3, False), (MMIN + 3 * 128 + 5, 768, 2, True), (MMIN + 3 * 128 + 5, 256, 1, False)]
_CACHE = {}


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def sample_rows(M):
    """About 96 rows: twelve of the sixteen rows of EACH of the eight waves (row offsets 0, 16, ..., 112 inside a 128-row
    block), two waves each in the first block, in two blocks in between and in the last whole block, the window of twelve
    moving through the sixteen lanes from wave to wave; behind them whatever rows the last, partial block holds of its last
    16-row group."""
    nblk = M // 128                                             # whole blocks
    blocks = [0, 0, nblk // 3, nblk // 3, 2 * nblk // 3, 2 * nblk // 3, nblk - 1, nblk - 1]
    rows = [np.arange(12) + (128 * b + 16 * wave + (4 * wave) % 5) for wave, b in enumerate(blocks)]
    if M % 128:
        rows.append(np.arange((M - 1) // 16 * 16, M))
    return np.unique(np.concatenate(rows))


class _Problem:
    """one shape: the gradient, the weights, both kinds of x, the residual (made and sent once), the float64 reference"""

    def __init__(self, M, kb, nb, neg):
        L, hp = _lib_hp()
        self.L, self.hp, self.M, self.kb, self.nb, self.K = L, hp, M, kb, nb, kb * nb
        rng = np.random.default_rng(M + self.K)
        K = self.K
        self.a = rng.standard_normal((M, K), dtype=np.float32)
        self.zero_rows = [0, M // 2 + 3, M - 1]
        self.a[self.zero_rows] = 0.0
        self.w = (rng.standard_normal((D, K), dtype=np.float32) / np.float32(np.sqrt(K)))
        self.wn = rng.uniform(0.5, 1.5, D).astype(np.float32)
        self.ex = rng.standard_normal((M, D), dtype=np.float32)
        self.dw0 = rng.standard_normal(D).astype(np.float32)
        x = rng.standard_normal((M, D), dtype=np.float32)
        self.x = {"normal": x, "rowscaled": x * (10.0 ** rng.uniform(-3, 3, M)).astype(np.float32)[:, None]}
        self.rms = {k: np.sqrt((v.astype(np.float64) ** 2).mean(-1) + 1e-6).astype(np.float32) for k, v in self.x.items()}
        self.rows = sample_rows(M)
        # the weights where the entry reads them: nb blocks (288 x kb), 64 floats further apart than they are large
        step = D * kb + 64
        blocks = np.zeros((nb, step), np.float32)
        for i in range(nb):
            blocks[(nb - 1 - i) if neg else i, :D * kb] = self.w[:, i * kb:(i + 1) * kb].reshape(-1)
        self.wd = hp.from_numpy(blocks)
        self.w0 = self.wd._ptr + (4 * step * (nb - 1) if neg else 0)
        self.bstride = -step if neg else step
        self.ad, self.exd, self.wnd = hp.from_numpy(self.a), hp.from_numpy(self.ex), hp.from_numpy(self.wn)
        self.xd = {k: hp.from_numpy(v) for k, v in self.x.items()}
        self.rmsd = {k: hp.from_numpy(v) for k, v in self.rms.items()}
        self.dxn = hp.empty((M, D), np.float32)
        self.nws = L.query("pdn_rmsnorm_bwd_workspace_bytes", M, D)
        self.nwsd = hp.empty((self.nws,), np.bool_)
        self.fws = L.query("pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes", M, kb, nb)
        self.fwsd = hp.empty((self.fws,), np.bool_)
        self.dy64 = self.a.astype(np.float64) @ self.w.astype(np.float64).T              # once per shape, all rows
        self._ref = {}

    def reference(self, kind, with_ex):
        """float64: dx on the sampled rows, dw over all rows"""
        if kind not in self._ref:
            z = self.x[kind].astype(np.float64) / self.rms[kind].astype(np.float64)[:, None]
            dw = (self.dy64 * z).sum(0)
            r = self.rows
            dz = self.dy64[r] * self.wn.astype(np.float64)
            dx = (dz - z[r] * (z[r] * dz).mean(-1, keepdims=True)) / self.rms[kind].astype(np.float64)[r, None]
            self._ref[kind] = (dx, dw)
        dx, dw = self._ref[kind]
        return (dx + self.ex[self.rows] if with_ex else dx), dw

    def _outputs(self, dw_mode):
        hp = self.hp
        dx = hp.from_numpy(np.full((self.M + 16, D), CANARY, np.float32))
        dw = None if dw_mode is None else hp.from_numpy(self.dw0 if dw_mode == "+=" else np.full(D, CANARY, np.float32))
        return dx, dw

    def fused(self, kind, with_ex, dw_mode):
        L, hp = self.L, self.hp
        dx, dw = self._outputs(dw_mode)
        L.call(ENTRY, self.ad._ptr, self.w0, self.bstride, self.kb, self.nb, self.xd[kind]._ptr, self.wnd._ptr,
               self.rmsd[kind]._ptr, self.exd._ptr if with_ex else None, dx._ptr, dw._ptr if dw is not None else None,
               1 if dw_mode == "+=" else 0, self.M, self.K, self.fwsd._ptr, self.fws, hp.stream())
        return dx.get(), (dw.get() if dw is not None else None)

    def pair(self, kind, with_ex, dw_mode):
        L, hp = self.L, self.hp
        dx, dw = self._outputs(dw_mode)
        L.call("pdn_gemm_outres_blocks_nt_f32", self.ad._ptr, self.w0, self.bstride, self.kb, self.nb, self.dxn._ptr, None,
               self.M, self.K, D, hp.stream())
        L.call("pdn_rmsnorm_bwd_f32", self.xd[kind]._ptr, self.wnd._ptr, self.rmsd[kind]._ptr, self.dxn._ptr,
               self.exd._ptr if with_ex else None, dx._ptr, dw._ptr if dw is not None else None,
               1 if dw_mode == "+=" else 0, self.M, D, self.nwsd._ptr, self.nws, hp.stream())
        return dx.get(), (dw.get() if dw is not None else None)


def _problem(shape):
    if shape not in _CACHE:
        _CACHE.clear()                       # one shape's arrays at a time
        _CACHE[shape] = _Problem(*shape)
    return _CACHE[shape]


def test_sampled_rows_cover_every_wave_and_the_block_range():
    for M, _, _, _ in SHAPES + [(57344, 0, 0, 0), (4096, 0, 0, 0)]:
        rows = sample_rows(M)
        assert 96 <= len(rows) <= 112 and rows.min() >= 0 and rows.max() < M
        assert {int(r) % 128 // 16 for r in rows} == set(range(8))           # all eight waves
        assert {int(r) % 16 for r in rows} == set(range(16))                 # all sixteen lanes r
        nblk = -(-M // 128)
        assert {0, nblk - 1} <= {int(r) // 128 for r in rows} and len({int(r) // 128 for r in rows}) >= 4
        if M % 128:
            assert M - 1 in rows


def _launches(L):
    return L.query("pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches", 0)


@pytest.mark.parametrize("with_ex", [False, True], ids=["noex", "ex"])
@pytest.mark.parametrize("kind", ["normal", "rowscaled"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"M{s[0]}_kb{s[1]}x{s[2]}")
def test_fused_against_float64_and_the_two_launches(hip, shape, kind, with_ex):
    P = _problem(shape)
    L, M, rows = P.L, P.M, P.rows
    ref_dx, ref_dw = P.reference(kind, with_ex)
    sdx, sdw = float(np.abs(ref_dx).max()), float(np.abs(ref_dw).max())
    for dw_mode in (None, "=", "+="):
        n0 = _launches(L)
        fdx, fdw = P.fused(kind, with_ex, dw_mode)
        assert _launches(L) - n0 == 1
        fdx2, fdw2 = P.fused(kind, with_ex, dw_mode)
        assert fdx.tobytes() == fdx2.tobytes(), "dx: two calls differ"
        pdx, pdw = P.pair(kind, with_ex, dw_mode)
        assert np.all(fdx[M:] == CANARY), "rows >= M of dx written"
        e_f = float(np.abs(fdx[rows] - ref_dx).max()) / sdx
        e_p = float(np.abs(pdx[rows] - ref_dx).max()) / sdx
        line = f"M={M} K={P.K} x={kind} ex={int(with_ex)} dw={dw_mode}: dx fused {e_f:.3e} pair {e_p:.3e}"
        if not with_ex:                      # an all-zero gradient row: dx is exactly zero
            assert not fdx[P.zero_rows].any()
        w_f = w_p = 0.0
        if dw_mode is not None:
            assert fdw.tobytes() == fdw2.tobytes(), "dw: two calls differ"
            want = ref_dw + (P.dw0 if dw_mode == "+=" else 0.0)
            w_f = float(np.abs(fdw - want).max()) / sdw
            w_p = float(np.abs(pdw - want).max()) / sdw
            line += f"; dw fused {w_f:.3e} pair {w_p:.3e}"
        print(line)
        assert e_f <= 2 * e_p + 1e-7, line
        assert w_f <= 2 * w_p + 1e-7, line


def test_switch_off_equals_the_two_launches_bit_for_bit(hip):
    P = _problem(SHAPES[0])
    n0 = _launches(P.L)
    with _env("PDN_NORM_BWD_FUSE", "0"):
        odx, odw = P.fused("normal", True, "+=")
    assert _launches(P.L) == n0
    pdx, pdw = P.pair("normal", True, "+=")
    assert odx.tobytes() == pdx.tobytes() and odw.tobytes() == pdw.tobytes()
    fdx, _ = P.fused("normal", True, "+=")              # read on every call: the split route again
    assert _launches(P.L) == n0 + 1


@pytest.mark.parametrize("M", [57344, 4096])
def test_below_the_split_kernels_rows(hip, M):
    P = _Problem(M, 288, 3, False)
    _CACHE.clear()
    L = P.L
    assert L.query("pdng_outres_blocks_nt_rmsnorm_bwd_supported", M, 288, 3) == 1
    n0 = _launches(L)
    fdx, fdw = P.fused("normal", True, "=")
    assert _launches(L) == n0
    if L.query("pdn_gemm_outres_blocks_supported", M, 288, 3):
        pdx, pdw = P.pair("normal", True, "=")
    else:                                # (trivially equal: see the docstring)
        with _env("PDN_NORM_BWD_FUSE", "0"):
            pdx, pdw = P.fused("normal", True, "=")
    assert fdx.tobytes() == pdx.tobytes() and fdw.tobytes() == pdw.tobytes()
    ref_dx, ref_dw = P.reference("normal", True)
    # fp32 against float64: a dot product of K = 864 terms and a sum over M rows carry about eps sqrt(n) of their scale,
    # 1.8e-6 and (M = 57344) 1.4e-5 at eps = 6e-8; the bounds are those, times five for dx (three roundings follow the
    # product) and times two for dw
    assert np.abs(fdx[P.rows] - ref_dx).max() <= 1e-5 * np.abs(ref_dx).max()
    assert np.abs(fdw - ref_dw).max() <= 3e-5 * np.abs(ref_dw).max()
    assert np.all(fdx[M:] == CANARY)
