"""The down-projection weight gradient dW_down (M x 288) = h^T g2 on split-fp16 MFMA (csrc/outres_tn_split.hip: the packed
kernel with the roles swapped, one block, transposed store) against float64 and against the fp32 wave-streaming kernel it
replaces from 32768 tokens up.  Both run through pdn_gemm_f32 in the form of the backward pass (core/fused/ffn.py:
`gemm(h.T, g2, wd.grad, beta=1)`): the split form when the workspace holds the extra region behind the 64 slabs (counter
slot 50 == 1, slot 42 == 0), the fp32 kernel when the workspace is the 64 slabs only (slot 50 == 0) -- the in-process A/B
switch of include/pdn_hip.h.

Figure: max |err| / (max_t |h[t, f]| * max_t |g2[t, d]|) against float64 over sampled groups of sixteen output rows f (a
wave's columns of h, which share the running exponent: the first, the last and two more) and all 288 columns d.  Criterion:
split <= 2 x the fp32 kernel's figure on the same inputs (the rule of tests/test_outres_tn_split_gpu.py).

Shapes (K, M, token stride of h, token stride of g2): 768 rows contiguous at the threshold; 768 rows with padded strides and
a short last range (1027 pieces in ranges of 25); 592 = 16 x 37 rows (five column workgroups, three idle waves in the last,
clamped column fetches) at both K.  g2 carries a column at 1e-6 of the others (17) and an all-zero column (33) throughout.
The row scalings are applied to h.

The image test restates the plane image of include/pdn_hip.h in NumPy and compares the bytes a split call left in the
caller's workspace: it passed unchanged on the library before and after the plane pass was rewritten for whole lines.

Measured on an MI355X over the twenty cases (every case prints its figures, profiles/down_dw_split_gpu_tests.txt): split
9.5e-7 .. 4.2e-6 against the fp32 kernel's 1.8e-6 .. 6.2e-6, below it in nineteen cases and 1.03 x it in one; the two-layer
step: the same loss, gradients within 5.0e-7 of their largest entry."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 288
KMIN = 32768
D_TINY, D_ZERO = 17, 33
CANARY = np.float32(7.5)
SLOTS = 51
SHAPES = [(KMIN, 768, 768, 288), (KMIN + 96, 768, 768 + 64, 288 + 32), (KMIN, 592, 592, 288), (KMIN + 96, 592, 592, 288)]
KINDS = ["flat", "loguniform", "rising", "falling", "tiny"]
_CACHE = {}


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    buf = (ctypes.c_int64 * SLOTS)()
    L.call("pdn_kernel_counters", buf, SLOTS, 1 if reset else 0)
    return list(buf)


def _extra(K):
    return (K // 32) * 36864 + 1152                      # the closed formula of include/pdn_hip.h


def _slabs(M):
    return 64 * M * D * 4


def _row_scale(kind, K, rng):
    if kind == "flat":
        return np.ones(K)
    if kind == "loguniform":
        return 10.0 ** rng.uniform(-6, 0, K)
    if kind == "rising":
        return 10.0 ** np.linspace(-8, 3, K)
    if kind == "falling":
        return 10.0 ** np.linspace(3, -8, K)
    assert kind == "tiny"
    return np.full(K, 1e-30)


def _ranges(M, K):
    """K ranges in use: ots_t_ranges / ots_k_per_split of csrc/split_tn_index.h"""
    pieces = K // 32
    r = min(64, 256 // (-(-M // 128)), pieces)
    kps = -(-pieces // r) * 32
    return -(-K // kps)


class _Problem:
    """g2 and unit-scale h of one shape (made once), the sampled rows, and both paths of the entry"""

    def __init__(self, K, M, ldh, ldg2):
        L, hp = _lib_hp()
        self.L, self.hp, self.K, self.M, self.ldh, self.ldg2 = L, hp, K, M, ldh, ldg2
        rng = np.random.default_rng(K + M)
        self.g2 = np.full((K, ldg2), 1e30, np.float32)                     # the padding must reach no output
        self.g2[:, :D] = rng.standard_normal((K, D), dtype=np.float32) * np.exp2(rng.integers(-3, 4, D)).astype(np.float32)
        self.g2[:, D_TINY] *= np.float32(1e-6)
        self.g2[:, D_ZERO] = 0.0
        a, b = rng.standard_normal((K, M), dtype=np.float32), rng.standard_normal((K, M), dtype=np.float32)
        self.h0 = a / (1.0 + np.exp(-a)) * b                               # SwiGLU of unit normals
        self.g2d = hp.from_numpy(self.g2)
        groups = sorted({0, 5, M // 16 - 7, M // 16 - 1})
        self.rows = np.concatenate([np.arange(16 * gi, 16 * gi + 16) for gi in groups])
        self.g64 = self.g2[:, :D].astype(np.float64)
        self.gmax = np.abs(self.g64).max(0)
        self.full = L.query("pdn_gemm_f32_workspace_bytes", M, D, K, 1)
        assert self.full == ((_slabs(M) + 255) & ~255) + _extra(K)
        self.ws = hp.empty((self.full // 4 + 1024,), np.float32)

    def h_dev(self, h):
        buf = np.full((self.K, self.ldh), 1e30, np.float32)
        buf[:, :self.M] = h
        return self.hp.from_numpy(buf)

    def run(self, hd, split, g2d=None, beta=0.0, prefill=0.0, keep_ws=False):
        """dW_down (M, 288) and the counters (slot 50, slot 42, slot 15) of one call; canaries checked"""
        L, hp, K, M = self.L, self.hp, self.K, self.M
        c = np.full((M + 1, D), CANARY, np.float32)                        # a canary row behind the output
        c[:M] = prefill
        cd = hp.from_numpy(c)
        self.ws[...] = float(CANARY)
        g2d = self.g2d if g2d is None else g2d
        wsb = self.full if split else _slabs(M)
        _counters(L, True)
        L.call("pdn_gemm_f32", M, D, K, 1.0, hd._ptr, 1, self.ldh, g2d._ptr, self.ldg2, 1, float(beta), cd._ptr, D, None,
               1, 1, 0, 0, 0, 0, 0, 0, None, None, 0, self.ws._ptr, wsb, hp.stream())
        cnt = _counters(L, True)
        out = cd.get()
        assert (out[M] == CANARY).all(), "a store behind the output"
        w = self.ws.get()
        assert (w[self.full // 4:] == CANARY).all(), "a store behind the workspace"
        if split:                                                          # behind the slabs in use, up to the images
            assert (w[_ranges(M, K) * M * D:_slabs(M) // 4] == CANARY).all(), "a store behind the last slab"
        else:
            assert (w[_slabs(M) // 4:] == CANARY).all(), "a store behind the slabs"
        if keep_ws:
            self.last_ws = w
        return out[:M], (cnt[50], cnt[42], cnt[15])

    def fig(self, out, h):
        """worst error of the sampled rows over max|h[:, f]| max|g2[:, d]|; a zero scale wants an exact zero"""
        h64 = h[:, self.rows].astype(np.float64)
        ref = h64.T @ self.g64
        scale = np.abs(h64).max(0)[:, None] * self.gmax[None, :]
        err = np.abs(out[self.rows].astype(np.float64) - ref)
        assert (err[scale == 0] == 0).all()
        return float((err[scale > 0] / scale[scale > 0]).max())


def _problem(i):
    if i not in _CACHE:
        _CACHE.clear()                                                     # one shape's buffers at a time
        _CACHE[i] = _Problem(*SHAPES[i])
    return _CACHE[i]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_split_down_gradient_at_fp32_accuracy(hip, shape, kind):
    p = _problem(shape)
    h = (p.h0 * _row_scale(kind, p.K, np.random.default_rng(7))[:, None]).astype(np.float32)
    hd = p.h_dev(h)
    out_s, cnt = p.run(hd, True)
    assert cnt == (1, 0, 0), cnt
    out_f, cnt = p.run(hd, False)
    assert cnt == (0, 0, 0), cnt
    fs, ff = p.fig(out_s, h), p.fig(out_f, h)
    print(f"K {p.K} M {p.M} (ldh {p.ldh}, ldg2 {p.ldg2}) {kind}: split {fs:.3e}, fp32 kernel {ff:.3e}")
    assert np.isfinite(out_s).all()
    assert (out_s[:, D_ZERO] == 0).all()
    assert fs <= 2.0 * ff, (fs, ff)


@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_accumulation_determinism_zero_and_nan(hip, shape):
    p = _problem(shape)
    K, M = p.K, p.M
    h = p.h0
    hd = p.h_dev(h)
    # ---- beta = 1 onto a non-zero C, and a bit-identical second launch ---------------------------------------------------
    base, cnt = p.run(hd, True)
    assert cnt == (1, 0, 0), cnt
    acc, cnt = p.run(hd, True, beta=1.0, prefill=3.0)
    assert cnt == (1, 0, 0), cnt
    again, _ = p.run(hd, True, beta=1.0, prefill=3.0)
    assert (acc == again).all()
    assert (acc == (base + np.float32(3.0))).all()                        # the reduce adds beta * C last, one fp32 add
    # ---- the all-zero column of g2 is exactly zero (the column at 1e-6 is measured on its own scale by fig) -------------
    assert (base[:, D_ZERO] == 0).all() and (base[:, D_TINY] != 0).all()
    # ---- an all-zero h ---------------------------------------------------------------------------------------------------
    out, cnt = p.run(p.h_dev(np.zeros_like(h)), True)
    assert cnt == (1, 0, 0) and (out == 0).all()
    # ---- a NaN in h marks only its output row, in both forms -------------------------------------------------------------
    fn = M - 21
    hn = h.copy()
    hn[K // 2 + 5, fn] = np.nan
    for split in (True, False):
        out, _ = p.run(p.h_dev(hn), split)
        bad = np.isnan(out)
        assert bad[fn].all() and bad.sum() == D, (split, int(bad.sum()))


def test_family_4_is_counted_once(hip):
    p = _problem(0)
    L = p.L
    hd = p.h_dev(p.h0)
    ms, fl, n = (ctypes.c_double * 5)(), (ctypes.c_double * 5)(), (ctypes.c_int64 * 5)()
    L.call("pdn_gemm_prof_collect_families", ms, fl, n)                   # (drains what earlier tests may have left)
    L.call("pdn_gemm_prof_enable", 1)
    try:
        p.run(hd, True)
    finally:
        L.call("pdn_gemm_prof_enable", 0)
    L.call("pdn_gemm_prof_collect_families", ms, fl, n)
    assert list(n) == [0, 0, 0, 0, 1], list(n)
    assert fl[4] == 2.0 * D * p.M * p.K


def test_workspace_sizes(hip):
    """sizes only: at 131072 tokens the benchmark's call is offered both regions whole under hipnp.gemm's cap of 1 << 28;
    below the threshold, for other widths and for the 288 x 288 product the answer stays the 64 slabs"""
    L, _ = _lib_hp()
    q = lambda M, N, K, nb=1: L.query("pdn_gemm_f32_workspace_bytes", M, N, K, nb)
    need = q(768, D, 131072)
    assert need == _slabs(768) + _extra(131072) and min(need, 1 << 28) == need
    assert q(768, D, KMIN - 32) == _slabs(768) and q(768, D, KMIN + 16) == _slabs(768)
    assert q(288, D, 131072) == 64 * 288 * D * 4 and q(776, D, 131072) == 64 * 776 * D * 4
    assert q(768, 320, 131072) == 64 * 768 * 320 * 4 and q(1040, D, 131072) == 64 * 1040 * D * 4


def _image(g2, K):
    """the extra region of include/pdn_hip.h for x = g2 (K x 288 float32): per piece of 32 tokens plane h, then plane l, each
    288 x 4 units of 8 halves (tokens 8 q .. 8 q + 7 of column d at unit 4 d + (q ^ ((d >> 2) & 3))); then 288 exponents"""
    amax = np.abs(g2).max(0)
    _, E = np.frexp(amax)
    sh = np.where(np.isfinite(amax) & (amax > 0), 9 - E, 0).astype(np.int32)       # the largest magnitude into [2^8, 2^9)
    s = np.ldexp(g2, sh[None, :]).astype(np.float32)
    hi = s.astype(np.float16)
    lo = ((s - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    npieces = K // 32
    img = np.zeros((npieces, 2, 288 * 4, 8), np.float16)
    d = np.arange(288)
    for q in range(4):
        u = 4 * d + (q ^ ((d >> 2) & 3))
        for plane, v in ((0, hi), (1, lo)):
            img[:, plane, u, :] = v.reshape(npieces, 4, 8, 288)[:, q].transpose(0, 2, 1)
    return img.reshape(-1).view(np.uint8), sh


def test_plane_image_bytes(hip):
    """K = threshold, padded ldx: the image region of the caller's workspace after a split call, byte for byte"""
    _CACHE.clear()
    p = _Problem(KMIN, 768, 768, 288 + 32)
    p.run(p.h_dev(p.h0), True, keep_ws=True)
    xoff = (_slabs(p.M) + 255) & ~255
    got = p.last_ws.view(np.uint8)[xoff:xoff + _extra(p.K)]
    want, sh = _image(p.g2[:, :D], p.K)
    assert sh[D_ZERO] == 0 and sh[D_TINY] >= sh.max() - 1 and sh[D_TINY] > 20
    nimg = (p.K // 32) * 36864
    assert np.array_equal(got[nimg:].view(np.int32), sh)
    diff = np.flatnonzero(got[:nimg] != want)
    assert diff.size == 0, (diff.size, diff[:8])
    print(f"K {p.K}, ldx {p.ldg2}: {nimg} image bytes and 288 exponents equal the restatement")


def test_training_step_route_on_and_off(hip):
    """one step of two layers at 32768 tokens: the same loss to seven digits and every gradient within 1e-4 of its largest
    entry (the batch gate's bound, as tests/test_rowtile_split_forms_gpu.py) between the split form and the fp32 kernel (the
    workspace size hipnp.gemm passes cut to the slabs)"""
    import builtins
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    L, hp = _lib_hp()
    _CACHE.clear()
    B, Lq = 128, 256
    rng = np.random.default_rng(3)
    ids, tgt = rng.integers(0, 512, (B, Lq)), rng.integers(0, 512, (B, Lq))
    emb = (0.02 * rng.standard_normal((512, 288))).astype(np.float32)

    def step(split):
        np.random.seed(0)
        model = Llama(512, 288, 6, 768, Lq, B, 2, np.float32)
        model.tok_embedding.weight.data[...] = emb                         # (the module leaves the table unset)
        model.to("hip:0")
        opt = Adam(model.parameters(), lr=0.0)
        _counters(L, True)
        real = L.call

        def call(name, *a):                                                # the slabs only: the in-process A/B switch
            if name == "pdn_gemm_f32" and not split and a[0] == 768 and a[1] == D and a[14] * a[15] == 1:
                a = a[:26] + (builtins.min(a[26], _slabs(768)),) + a[27:]
            return real(name, *a)
        L.call = call
        try:
            loss = model.finetune_step(ids, tgt, opt)
        finally:
            del L.call
        cnt = _counters(L, True)
        print(f"split {split}: slot 50 {cnt[50]}, slot 42 {cnt[42]}, slot 15 {cnt[15]}")
        return float(loss), {n: q.grad.get() for n, q in model.named_parameters()}, cnt

    loss_s, gs, cs = step(True)
    loss_f, gf, cf = step(False)
    assert cs[50] == 2 and cf[50] == 0, (cs[50], cf[50])                   # one product per layer
    assert cs[42] == cf[42] and cs[15] == cf[15]
    assert abs(loss_s - loss_f) <= 1e-7 * abs(loss_f), (loss_s, loss_f)
    worst = 0.0
    for name in gs:
        err = float(np.abs(gs[name] - gf[name]).max()) / max(float(np.abs(gf[name]).max()), 1e-12)
        worst = max(worst, err)
        assert err <= 1e-4, (name, err)
    print(f"loss {loss_s:.7f} against {loss_f:.7f}, worst gradient difference {worst:.3e} of its largest entry")
