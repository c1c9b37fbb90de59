"""The output-resident products C (M x 288) = A B + bias + residual on split-fp16 MFMA (csrc/outres_split.hip) against float64
and against the fp32 MFMA kernel they replace from 65536 rows up.  The split form runs behind the existing entries
(pdn_gemm_outres_blocks_nt_f32, pdn_gemm_outres_f32: counter slot 46 == 1, slot 14 == 1); PDN_OUTRES_SPLIT=0, read on every
call, keeps the fp32 kernel (slot 46 == 0).  The fp32 yardstick of the figures is taken through hipnp.gemm under
PDN_GEMM_NO_OUTRES=1, with packed weights for the block forms (tests/test_kernels_gpu.py holds the output-resident fp32
kernel to those bits).

Figure: max_d |err[t][d]| / (max_k |A[t][k]| * max_k |W[d][k]|) against float64, the worst of about 96 rows -- the first and
the last 16-row group (a wave's rows) of the first and of the last workgroup and two groups in between -- over all 288
columns, of the plain product (bias and residual are added in fp32 behind it; how is checked bit for bit in the second
test).  Criterion: split <= 2 x the fp32 kernel's figure on the same inputs; for the late outlier twice the figure of the
emulation with flushed fp16 subnormals (tests/test_outres_split_cpu.py) on the same rows.

Shapes, the smallest at which the path is taken: 65536 rows against 3 blocks of 288 (the benchmark's form, whole
workgroups); 65536 + 40 rows against 2 blocks of 768 at falling addresses with padded rows of A and C (ragged last row
block); 65536 + 16 rows against one matrix with K = 256 (the shortest K taken: fewer pieces than two ring turns); NN with
K = 768, residual and bias (the down projection); NN with K = 4096, residual only (the longest K taken).  Row-scale kinds
as in tests/test_outres_split_cpu.py; every W carries a row at 1e-6 of the others.

Measured on an MI355X over the forty cases (every case prints its figures): split 3.3e-7 .. 2.1e-5 against the fp32 kernel's
3.1e-7 .. 4.9e-5, below it in every case but one (K = 256, rising ramp: 1.06 x); the late outlier 2.8e-7 .. 3.8e-7 against
bounds of 3.9e-7 .. 6.0e-7."""
import ctypes
import os

import numpy as np
import pytest

from tests.test_outres_split_cpu import KINDS, emulate_split

pytestmark = pytest.mark.gpu

D = 288
MMIN = 65536
CANARY = np.float32(7.5)
# (M, form, blocks, falling addresses, lda - K, ldc - 288, K, residual, bias)
SHAPES = [(MMIN, "nt", 3, False, 0, 0, 864, True, False), (MMIN + 40, "nt", 2, True, 64, 32, 1536, True, False),
          (MMIN + 16, "nt", 1, False, 0, 0, 256, False, False), (MMIN, "nn", 1, False, 0, 32, 768, True, True),
          (MMIN, "nn", 1, False, 0, 0, 4096, True, False)]
_CACHE = {}


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    buf = (ctypes.c_int64 * 47)()
    L.call("pdn_kernel_counters", buf, 47, 1 if reset else 0)
    return list(buf)


class _env:
    """an environment variable for the calls inside, restored behind them"""

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


def _scaled(kind, a0, rng):
    """a copy of the unit-scale a0 with the row scales of `kind` (tests/test_outres_split_cpu.py: make_a), in fp32"""
    M, K = a0.shape
    if kind == "loguniform":
        return a0 * (10.0 ** rng.uniform(-6, 3, M)).astype(np.float32)[:, None]
    if kind == "rising":
        return a0 * (10.0 ** np.linspace(-8, 3, K)).astype(np.float32)[None, :]
    if kind == "falling":
        return a0 * (10.0 ** np.linspace(3, -8, K)).astype(np.float32)[None, :]
    if kind == "tiny":
        return a0 * np.float32(1e-30)
    a = a0.copy()
    if kind == "outlier":
        a[:, K - 40] *= np.float32(1e6)
    elif kind == "zero_row":
        a[::3] = 0.0
    elif kind == "half_zero":
        a[::3, :K // 2] = 0.0
    else:
        assert kind == "flat"
    return a


class _Problem:
    """the weights, residual and bias of one shape (made once), a unit-scale A, the sampled rows, and the ways to run it"""

    def __init__(self, M, form, nb, neg, lda_pad, ldc_pad, K, with_res, with_bias):
        L, hp = _lib_hp()
        self.L, self.hp, self.M, self.form, self.nb, self.neg, self.K = L, hp, M, form, nb, neg, K
        self.lda, self.ldc, self.kb = K + lda_pad, D + ldc_pad, K // nb
        rng = np.random.default_rng(M + K)
        self.w = rng.standard_normal((D, K), dtype=np.float32) * np.exp2(rng.integers(-3, 4, D)).astype(np.float32)[:, None]
        self.w[17] *= np.float32(1e-6)
        self.a0 = np.tile(rng.standard_normal((2048, K), dtype=np.float32), (-(-M // 2048), 1))[:M]
        self.res = rng.standard_normal((M, D), dtype=np.float32) if with_res else None
        self.bias = rng.standard_normal(D, dtype=np.float32) if with_bias else None
        nblk = -(-M // 128)
        last = (nblk - 1) * 128
        groups = [0, 112, 128 * (nblk // 3) + 48, 128 * (2 * nblk // 3) + 80, last, (M - 1) // 16 * 16]
        self.rows = np.unique(np.concatenate([np.arange(g, min(g + 16, M)) for g in groups]))
        self.set_w(self.w)
        self.resd = None
        if with_res:                                                       # in a buffer with C's row stride
            r = np.zeros((M, self.ldc), np.float32)
            r[:, :D] = self.res
            self.resd = hp.from_numpy(r)
        self.biasd = hp.from_numpy(self.bias) if with_bias else None

    def set_w(self, w):
        """the weights where the entry reads them (blocks 64 floats further apart than they are large), and packed for hipnp.gemm"""
        hp, nb, kb = self.hp, self.nb, self.kb
        if self.form == "nn":
            self.wd = hp.from_numpy(np.ascontiguousarray(w.T))            # B (K x 288)
            self.wpack = self.wd
            return
        step = D * kb + 64
        buf = np.full(nb * step, 1e30, np.float32)
        for b in range(nb):
            at = (nb - 1 - b if self.neg else b) * step
            buf[at:at + D * kb] = w[:, b * kb:(b + 1) * kb].ravel()
        self.wd = hp.from_numpy(buf)
        self.w0 = self.wd._ptr + 4 * ((nb - 1) * step if self.neg else 0)
        self.bstride = -step if self.neg else step
        self.wpack = hp.from_numpy(np.ascontiguousarray(w))               # (288, K): B = its transpose

    def a_dev(self, a):
        if self.lda == self.K:
            return self.hp.from_numpy(a)
        buf = np.full((self.M, self.lda), 1e30, np.float32)               # the padding must reach no output
        buf[:, :self.K] = a
        return self.hp.from_numpy(buf)

    def run(self, ad, split, res=False, bias=False):
        """one call of the entry -> (C (M x 288), (slot 14, slot 46)); the canaries behind C and in its padding checked"""
        L, hp, M = self.L, self.hp, self.M
        c = np.full((M + 1, self.ldc), CANARY, np.float32)
        cd = hp.from_numpy(c)
        rp = self.resd._ptr if res and self.resd is not None else None
        bp = self.biasd._ptr if bias and self.biasd is not None else None
        with _env("PDN_OUTRES_SPLIT", "1" if split else "0"):
            _counters(L, True)
            if self.form == "nt" and self.nb > 1:
                assert bp is None
                L.call("pdn_gemm_outres_blocks_nt_f32", ad._ptr, self.w0, self.bstride, self.kb, self.nb, cd._ptr, rp, M, self.lda,
                       self.ldc, hp.stream())
            elif self.form == "nt":
                L.call("pdn_gemm_outres_f32", ad._ptr, self.w0, cd._ptr, bp, rp, M, D, self.K, self.lda, self.K, self.ldc, 1, hp.stream())
            else:
                L.call("pdn_gemm_outres_f32", ad._ptr, self.wd._ptr, cd._ptr, bp, rp, M, D, self.K, self.lda, D, self.ldc, 0, hp.stream())
            cnt = _counters(L, True)
        out = cd.get()
        assert (out[M] == CANARY).all(), "a store behind C"
        assert (out[:M, D:] == CANARY).all(), "a store into the padding of C"
        return out[:M, :D], (cnt[14], cnt[46])

    def run_tiled(self, ad, res=False):
        """the same product on the fp32 pipe through hipnp.gemm, the output-resident kernels switched off"""
        hp = self.hp
        y = hp.empty((self.M, D), np.float32)
        av = ad if self.lda == self.K else ad[:, :self.K]
        r = None
        if res and self.resd is not None:
            r = hp.from_numpy(self.res)
        with _env("PDN_GEMM_NO_OUTRES", "1"):
            hp.gemm(av, self.wpack.T if self.form == "nt" else self.wpack, y, residual=r)
        return y.get()

    def fig(self, out, a, w=None):
        """worst sampled row of max_d |err| / (max_k |A[t]| max_k |W[d]|); a zero scale wants an exact zero"""
        w = self.w if w is None else w
        a64, w64 = a[self.rows].astype(np.float64), w.astype(np.float64)
        ref = a64 @ w64.T
        scale = np.abs(a64).max(1)[:, None] * np.abs(w64).max(1)[None, :]
        err = np.abs(out[self.rows].astype(np.float64) - ref)
        assert (err[scale == 0] == 0).all()
        return float((err[scale > 0] / scale[scale > 0]).max())


def _problem(i):
    if i not in _CACHE:
        _CACHE.clear()                                                     # one shape's buffers at a time
        _CACHE[i] = _Problem(*SHAPES[i])
    return _CACHE[i]


def _name(p):
    return f"M {p.M} {p.form} K {p.K} ({p.nb} blocks)"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_split_products_at_fp32_accuracy(hip, shape, kind):
    p = _problem(shape)
    a = _scaled(kind, p.a0, np.random.default_rng(7))
    ad = p.a_dev(a)
    out_s, cnt = p.run(ad, True)
    assert cnt == (1, 1), cnt
    fs, ff = p.fig(out_s, a), p.fig(p.run_tiled(ad), a)
    assert np.isfinite(out_s).all()
    if kind == "zero_row":
        assert (out_s[::3] == 0).all()
    if kind == "outlier":
        emu, moves = emulate_split(a[p.rows], p.w, True)
        assert (moves == 1).all()                                          # the rescale path ran in every sampled row
        a64, w64 = a[p.rows].astype(np.float64), p.w.astype(np.float64)
        scale = np.abs(a64).max(1)[:, None] * np.abs(w64).max(1)[None, :]
        bound = 2.0 * float((np.abs(emu.astype(np.float64) - a64 @ w64.T) / scale).max())
        print(f"{_name(p)} {kind}: split {fs:.3e}, fp32 kernel {ff:.3e}, bound (2 x flushed emulation) {bound:.3e}")
        assert fs <= bound, (fs, bound)
    else:
        print(f"{_name(p)} {kind}: split {fs:.3e}, fp32 kernel {ff:.3e}")
        assert fs <= 2.0 * ff, (fs, ff)


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_epilogue_determinism_zero_rows_nonfinite_and_switch(hip, shape):
    p = _problem(shape)
    hp, M, K = p.hp, p.M, p.K
    a = _scaled("zero_row", p.a0, np.random.default_rng(7))
    ad = p.a_dev(a)
    # ---- bias and residual are added in fp32 behind the product, in that order; a bit-identical second launch --------------
    plain, cnt = p.run(ad, True)
    assert cnt == (1, 1)
    full, cnt = p.run(ad, True, res=True, bias=True)
    assert cnt == (1, 1)
    again, _ = p.run(ad, True, res=True, bias=True)
    assert np.array_equal(full, again)
    want = plain
    if p.bias is not None:
        want = want + p.bias[None, :]
    if p.res is not None:
        want = want + p.res
    assert want.dtype == np.float32 and np.array_equal(full, want)
    # ---- an all-zero row comes out exactly as residual + bias ------------------------------------------------------------------
    zero = np.zeros((1, D), np.float32)
    if p.bias is not None:
        zero = zero + p.bias[None, :]
    zero = np.broadcast_to(zero, full[::3].shape)
    assert np.array_equal(full[::3], zero + p.res[::3] if p.res is not None else zero)
    # ---- the switch: slot 46 stays 0, the fp32 kernel's bits -------------------------------------------------------------------
    off, cnt = p.run(ad, False, res=True)
    assert cnt == (1, 0), cnt
    assert np.array_equal(off, p.run_tiled(ad, res=True))
    # ---- a NaN and an Inf in A mark their own rows only, a NaN in W its column only -----------------------------------------------
    rn, ri, dn = 128 * 5 + 37, M - 3, 100
    an = p.a0.copy()
    an[rn, K // 2 + 3] = np.nan
    an[ri, 7] = np.inf
    out, _ = p.run(p.a_dev(an), True)
    bad = ~np.isfinite(out)
    assert bad[rn].all() and bad[ri].all() and bad.sum() == 2 * D, int(bad.sum())
    wn = p.w.copy()
    wn[dn, K - 9] = np.nan
    p.set_w(wn)
    try:
        out, _ = p.run(p.a_dev(p.a0), True)
    finally:
        p.set_w(p.w)
    bad = np.isnan(out)
    assert bad[:, dn].all() and bad.sum() == M, int(bad.sum())


def test_fewer_rows_keep_the_fp32_kernel(hip):
    L, hp = _lib_hp()
    M, K = MMIN - 128, 864
    rng = np.random.default_rng(5)
    ad = hp.from_numpy(rng.standard_normal((M, K), dtype=np.float32))
    wd = hp.from_numpy(rng.standard_normal((D, K), dtype=np.float32))
    cd = hp.empty((M, D), np.float32)
    _counters(L, True)
    L.call("pdn_gemm_outres_f32", ad._ptr, wd._ptr, cd._ptr, None, None, M, D, K, K, K, D, 1, hp.stream())
    cnt = _counters(L, True)
    assert (cnt[14], cnt[46]) == (1, 0), (cnt[14], cnt[46])


def test_training_step_split_on_and_off(hip):
    """one step of two layers at 65536 tokens: the losses agree to 1e-6 relative and every gradient within 1e-4 of its
    largest entry (the batch gate's bound) between the split form and the fp32 kernel"""
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    L, hp = _lib_hp()
    B, Lq = 256, 256
    rng = np.random.default_rng(3)
    ids, tgt = rng.integers(0, 512, (B, Lq)), rng.integers(0, 512, (B, Lq))
    emb = (0.02 * rng.standard_normal((512, 288))).astype(np.float32)

    def step(split):
        np.random.seed(0)
        model = Llama(512, 288, 6, 768, Lq, B, 2, np.float32)
        model.tok_embedding.weight.data[...] = emb                         # (the module leaves the table unset)
        model.to("hip:0")
        opt = Adam(model.parameters(), lr=0.0)
        with _env("PDN_OUTRES_SPLIT", "1" if split else "0"):
            _counters(L, True)
            loss = model.finetune_step(ids, tgt, opt)
            cnt = _counters(L, True)
        print(f"split {split}: slot 14 {cnt[14]}, slot 46 {cnt[46]}")
        return float(loss), {n: q.grad.get() for n, q in model.named_parameters()}, cnt[46]

    loss_s, gs, n_s = step(True)
    loss_f, gf, n_f = step(False)
    assert n_s == 6 and n_f == 0, (n_s, n_f)                               # two input gradients and a down projection per layer
    assert abs(loss_s - loss_f) <= 1e-6 * abs(loss_f), (loss_s, loss_f)
    for name in gs:
        err = float(np.abs(gs[name] - gf[name]).max()) / max(float(np.abs(gf[name]).max()), 1e-12)
        assert err <= 1e-4, (name, err)
