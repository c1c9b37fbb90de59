"""The 288 x 288 products of a training step -- the attention output projection ctx Wo + x (NN, residual) and its input
gradient dz Wo^T (NT) -- at 65536 rows and more.  pdn_gemm_f32 sends them to the split-fp16 output-resident kernel
(csrc/outres_split.hip, nine pieces of 32) instead of the fp32 tile-piece kernel gemm_rowtile_kernel<.., 0 / 6>: the
output-resident route measured faster than the fp32 kernel at K = 288, so no EPI 0 / 6 form of
rts_main_kernel was added.  Counter slot 47 counts the route and nothing else does; pdn_gemm_rowtile_mode(3) keeps the fp32
tile-piece kernel (slot 1), which is the yardstick here.

Shapes, the smallest the route takes: M in {65536, 65536 + 37 (ragged last row block)}; NN with residual, NT with bias, and
once A, C and the residual as column blocks of wider buffers.  Reference: float64 on about 100 sampled and special rows.
Criterion: worst over the rows of max_d |err| / max_d |output| of the split form <= 2 x the fp32 kernel's on
the same inputs.  Special rows: scaled by 3e5 and by 1e-7, one element 1e4 above its row, an all-zero row (bias + residual
exactly), a NaN row (NaN there and nowhere else); column 17 of W at 1e-6 of the others, judged at its own scale; a canary
row behind C and canary padding; a bit-identical second launch.  Every case prints its figures."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 288
MMIN = 65536
CANARY = np.float32(7.5)
SMALL_COL = 17
# (M, B given as its transpose, residual, bias, A / C / residual as column blocks of wider buffers)
CASES = [(MMIN, False, True, False, False), (MMIN + 37, False, True, False, True), (MMIN, True, False, True, False),
         (MMIN + 37, True, False, True, False)]
R_BIG, R_SMALL, R_OUT, R_ZERO = 3, 130, 261, 1029            # special rows (the same in every case)


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    buf = (ctypes.c_int64 * 48)()
    L.call("pdn_kernel_counters", buf, 48, 1 if reset else 0)
    return list(buf)


class _mode:
    """pdn_gemm_rowtile_mode for the calls inside, restored behind them"""

    def __init__(self, L, mode):
        self.L, self.mode = L, mode

    def __enter__(self):
        self.prev = self.L.query("pdn_gemm_rowtile_mode", self.mode)

    def __exit__(self, *exc):
        self.L.query("pdn_gemm_rowtile_mode", self.prev)


def _inputs(M, with_res, with_bias):
    rng = np.random.default_rng(M)
    w = rng.standard_normal((D, D), dtype=np.float32) * np.exp2(rng.integers(-3, 4, D)).astype(np.float32)[:, None]
    w[SMALL_COL] *= np.float32(1e-6)                             # w[d, k]: row d makes output column d
    a = np.tile(rng.standard_normal((2048, D), dtype=np.float32), (-(-M // 2048), 1))[:M]
    a[R_BIG] *= np.float32(3e5)
    a[R_SMALL] *= np.float32(1e-7)
    a[R_OUT, D - 40] *= np.float32(1e4)
    a[R_ZERO] = 0.0
    res = bias = None
    if with_res:
        res = rng.standard_normal((M, D), dtype=np.float32)
        res[[R_BIG, R_SMALL, R_OUT]] = 0.0                       # the scaled rows are judged on the product alone
        res[:, SMALL_COL] = 0.0                                  # ... and so is the small column
    if with_bias:
        bias = rng.standard_normal(D, dtype=np.float32)
        bias[SMALL_COL] = 0.0
    nblk = -(-M // 128)
    groups = [0, 112, 128 * (nblk // 3) + 48, 128 * (2 * nblk // 3) + 80, (nblk - 1) * 128, (M - 1) // 16 * 16]
    rows = np.unique(np.concatenate([np.arange(g, min(g + 16, M)) for g in groups] + [[R_BIG, R_SMALL, R_OUT, R_ZERO]]))
    return w, a, res, bias, rows


class _Case:
    def __init__(self, M, nt, with_res, with_bias, wide):
        L, hp = _lib_hp()
        self.L, self.hp, self.M, self.nt, self.wide = L, hp, M, nt, wide
        self.w, self.a, self.res, self.bias, self.rows = _inputs(M, with_res, with_bias)
        self.wd = hp.from_numpy(self.w if nt else np.ascontiguousarray(self.w.T))      # NT: (288 x K) as stored; NN: B (K x 288)
        self.biasd = hp.from_numpy(self.bias) if with_bias else None
        self.a_off, self.lda = (32, D + 64) if wide else (0, D)
        self.c_off, self.ldc = (64, D + 128) if wide else (0, D)
        self.resd = None
        if with_res:
            r = np.zeros((M, self.ldc), np.float32)
            r[:, self.c_off:self.c_off + D] = self.res
            self.resd = hp.from_numpy(r)

    def a_dev(self, a):
        buf = np.full((self.M, self.lda), 1e30, np.float32)                             # the padding must reach no output
        buf[:, self.a_off:self.a_off + D] = a
        return self.hp.from_numpy(buf)

    def run(self, ad, mode):
        """one hipnp.gemm under pdn_gemm_rowtile_mode `mode` -> (C (M x 288), counters); canaries checked"""
        L, hp, M = self.L, self.hp, self.M
        cd = hp.from_numpy(np.full((M + 1, self.ldc), CANARY, np.float32))
        av = ad[:, self.a_off:self.a_off + D]
        cv = cd[:M, self.c_off:self.c_off + D]
        rv = self.resd[:, self.c_off:self.c_off + D] if self.resd is not None else None
        with _mode(L, mode):
            _counters(L, True)
            hp.gemm(av, self.wd.T if self.nt else self.wd, cv, bias=self.biasd, residual=rv)
            cnt = _counters(L, True)
        out = cd.get()
        assert (out[M] == CANARY).all(), "a store behind C"
        assert (out[:M, :self.c_off] == CANARY).all() and (out[:M, self.c_off + D:] == CANARY).all(), "a store into the padding of C"
        return out[:M, self.c_off:self.c_off + D], cnt

    def ref64(self, a):
        ref = a[self.rows].astype(np.float64) @ self.w.astype(np.float64).T
        if self.bias is not None:
            ref = ref + self.bias.astype(np.float64)[None, :]
        if self.res is not None:
            ref = ref + self.res[self.rows].astype(np.float64)
        return ref

    def figs(self, out, ref):
        """(worst row of max_d |err| / max_d |ref|, the small column's max |err| / max |ref| over the rows)"""
        err = np.abs(out[self.rows].astype(np.float64) - ref)
        big = np.abs(ref).max(1)
        assert (err[big == 0] == 0).all()
        row = float((err.max(1)[big > 0] / big[big > 0]).max())
        plain = np.ones(len(self.rows), bool)                                           # (the scaled rows have scales of their own)
        plain[np.isin(self.rows, [R_BIG, R_SMALL, R_OUT])] = False
        col = float(err[plain, SMALL_COL].max() / np.abs(ref[plain, SMALL_COL]).max())
        return row, col


@pytest.mark.parametrize("case", range(len(CASES)))
def test_288_products_at_fp32_accuracy(hip, case):
    c = _Case(*CASES[case])
    ad = c.a_dev(c.a)
    out_s, cnt = c.run(ad, 1)
    assert (cnt[47], cnt[1], cnt[14], cnt[46]) == (1, 0, 0, 0), (cnt[47], cnt[1], cnt[14], cnt[46])
    out_f, cnt = c.run(ad, 3)
    assert (cnt[47], cnt[1], cnt[14], cnt[46]) == (0, 1, 0, 0), (cnt[47], cnt[1], cnt[14], cnt[46])
    ref = c.ref64(c.a)
    (rs, cs), (rf, cf) = c.figs(out_s, ref), c.figs(out_f, ref)
    print(f"M {c.M} {'NT' if c.nt else 'NN'}{' residual' if c.res is not None else ''}{' bias' if c.bias is not None else ''}"
          f"{' wide' if c.wide else ''}: worst row split {rs:.3e}, fp32 kernel {rf:.3e}; small column split {cs:.3e}, fp32 kernel {cf:.3e}")
    assert np.isfinite(out_s).all()
    assert rs <= 2.0 * rf, (rs, rf)
    assert cs <= 2.0 * cf, (cs, cf)
    # ---- the all-zero row is bias + residual exactly --------------------------------------------------------------------
    want = np.zeros(D, np.float32)
    if c.bias is not None:
        want = want + c.bias
    if c.res is not None:
        want = want + c.res[R_ZERO]
    assert np.array_equal(out_s[R_ZERO], want)
    # ---- a second launch gives the same bits ------------------------------------------------------------------------------
    again, _ = c.run(ad, 1)
    assert np.array_equal(out_s, again)
    # ---- a NaN marks its own row only ---------------------------------------------------------------------------------------
    rn = 128 * 5 + 37
    an = c.a.copy()
    an[rn, D // 2 + 3] = np.nan
    out_n, _ = c.run(c.a_dev(an), 1)
    bad = np.isnan(out_n)
    assert bad[rn].all() and bad.sum() == D, int(bad.sum())


def test_other_calls_keep_their_kernels(hip):
    """below 65536 rows, and at 65536 rows under PDN_OUTRES_SPLIT=0 (read on every call), the fp32 tile-piece kernel runs
    (slot 1) with the bits it has under pdn_gemm_rowtile_mode(3)"""
    import os
    L, hp = _lib_hp()
    rng = np.random.default_rng(5)
    a = rng.standard_normal((MMIN, D), dtype=np.float32)
    ad, wd = hp.from_numpy(a), hp.from_numpy(rng.standard_normal((D, D), dtype=np.float32))

    def run(M):
        cd = hp.empty((M, D), np.float32)
        _counters(L, True)
        hp.gemm(ad[:M], wd, cd)
        cnt = _counters(L, True)
        return cd.get(), (cnt[47], cnt[1])

    assert run(MMIN - 256)[1] == (0, 1)
    assert run(MMIN)[1] == (1, 0)
    old = os.environ.get("PDN_OUTRES_SPLIT")
    os.environ["PDN_OUTRES_SPLIT"] = "0"
    try:
        off, cnt = run(MMIN)
    finally:
        if old is None:
            del os.environ["PDN_OUTRES_SPLIT"]
        else:
            os.environ["PDN_OUTRES_SPLIT"] = old
    assert cnt == (0, 1), cnt
    with _mode(L, 3):
        ref, cnt = run(MMIN)
    assert cnt == (0, 1), cnt
    assert np.array_equal(off, ref)


def test_training_step_route_on_and_off(hip):
    """one step of two layers at 65536 tokens: the losses agree to 1e-6 relative and every gradient within 1e-4 of its
    largest entry (the batch gate's bound) between the default routes and pdn_gemm_rowtile_mode(3)"""
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    L, hp = _lib_hp()
    B, Lq = 256, 256
    rng = np.random.default_rng(3)
    ids, tgt = rng.integers(0, 512, (B, Lq)), rng.integers(0, 512, (B, Lq))
    emb = (0.02 * rng.standard_normal((512, 288))).astype(np.float32)

    def step(mode):
        np.random.seed(0)
        model = Llama(512, 288, 6, 768, Lq, B, 2, np.float32)
        model.tok_embedding.weight.data[...] = emb                         # (the module leaves the table unset)
        model.to("hip:0")
        opt = Adam(model.parameters(), lr=0.0)
        with _mode(L, mode):
            _counters(L, True)
            loss = model.finetune_step(ids, tgt, opt)
            cnt = _counters(L, True)
        print(f"mode {mode}: slot 47 {cnt[47]}, slot 1 {cnt[1]}, slot 3 {cnt[3]}, slot 46 {cnt[46]}")
        return float(loss), {n: q.grad.get() for n, q in model.named_parameters()}, cnt

    loss_s, gs, cs = step(1)
    loss_f, gf, cf = step(3)
    assert cs[47] == 4 and cf[47] == 0, (cs[47], cf[47])                   # the output projection and its input gradient per layer
    assert cs[3] == cf[3] == 2 and cs[46] == cf[46] == 6, (cs[3], cf[3], cs[46], cf[46])
    assert abs(loss_s - loss_f) <= 1e-6 * abs(loss_f), (loss_s, loss_f)
    worst = 0.0
    for name in gs:
        err = float(np.abs(gs[name] - gf[name]).max()) / max(float(np.abs(gf[name]).max()), 1e-12)
        worst = max(worst, err)
        assert err <= 1e-4, (name, err)
    print(f"loss {loss_s:.7f} against {loss_f:.7f}, worst gradient difference {worst:.3e} of its largest entry")
