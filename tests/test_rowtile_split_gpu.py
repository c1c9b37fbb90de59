"""The q | k | v + RoPE and gate | up + SwiGLU projections on split-fp16 MFMA (csrc/rowtile_split.hip: the form the four
`pdn_{qkv_rope,gateup_swiglu}[_norm]_fwd_f32` entries take at 16384 rows and more) against float64 and against the fp32 MFMA
kernel they replace there (the same entry under `pdn_gemm_rowtile_mode(3)`).  llm/llama/model.py:23-44, 56-58, 93-104 with
the RMSNorm of nn/modules/norm.py:221-248 folded in.

Criterion (the one of tests/test_lm_head_split_gpu.py): the worst row error relative to the row's largest |output| -- float64
reference on about 60 sampled rows plus the special rows -- of the split kernel is at most 2 x that of the fp32 kernel on the
same inputs, for qkv, gu and h each.  The factor 2 only allows for a different summation order (tests/test_rowtile_split_cpu.py:
the arithmetic is at parity with an fp32 product).  xn and rms against float64 at the 2e-6 of tests/test_fused_epilogues.py,
taken per row.

Shapes: M in {16384 (columns cut over grid.y), 16384 + 37 (GUARD form), 65536 (one uncut workgroup per CU)}.  The q | k | v
entries want M to be a multiple of the sequence length, itself a multiple of 32, so their GUARD shape is 16384 + 64 with
L = 64; with L = 256 every valid M is a multiple of 256.  The entries fix the outputs' leading dimensions (3 D, 2 F, F, K), so
the wider leading dimension is x's (K + 8, the padding holds a canary that must not reach any output), and the outputs carry
eight canary rows past M that must stay untouched.

Special rows / columns: rows scaled by 3e5 and by 1e-7, a row with one 1e4 outlier, an all-zero row (rms = sqrt(eps), outputs
zero), a column of 1e-6-sized weights, a NaN in the last row (that row NaN in every output, no other).

Measured on an MI355X over the thirteen cases (every case prints its figures): gu split 3.3e-7 .. 4.9e-7 against the fp32
kernel's 8.2e-7 .. 1.06e-6; h 4.5e-7 .. 6.3e-7 against 9.7e-7 .. 1.88e-6; qkv 3.0e-7 .. 4.6e-7 against 7.3e-7 .. 8.8e-7.  One
training step (2 layers, 16384 tokens): the loss agrees to all printed digits (5.2128386)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = D = 288
EPS = 1e-6
R_BIG, R_SMALL, R_OUTLIER, R_ZERO, C_TINY = 3, 5, 7, 9, 17
CANARY = np.float32(7.5)
PAD = 8


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _counters(L, reset):
    buf = (ctypes.c_int64 * 42)()
    L.call("pdn_kernel_counters", buf, 42, 1 if reset else 0)
    return list(buf)


def _rows(M):
    return np.unique(np.concatenate([[R_BIG, R_SMALL, R_OUTLIER, R_ZERO, 0, M - 2], np.random.default_rng(1).integers(0, M - 1, 60)]))


def _x(M, rng):
    """(M, K + 8) with the payload in the first K columns and a canary (1e30) in the padding."""
    x = np.full((M, K + PAD), 1e30, np.float32)
    x[:, :K] = rng.standard_normal((M, K), dtype=np.float32) * rng.uniform(0.2, 3.0, (M, 1)).astype(np.float32)
    x[R_BIG, :K] *= np.float32(3e5)
    x[R_SMALL, :K] *= np.float32(1e-7)
    x[R_OUTLIER, 11] = 1e4
    x[R_ZERO, :K] = 0.0
    x[M - 1, 100] = np.nan
    return x


def _norm64(x, wn):
    x64 = x.astype(np.float64)
    r = np.sqrt((x64 * x64).mean(-1) + EPS)
    return x64 / r[:, None] * wn.astype(np.float64), r


def _worst(got, ref):
    """worst over the rows of max |err| / max |output| (a row of zeros: its error must be zero)."""
    err, scale = np.abs(got.astype(np.float64) - ref).max(1), np.abs(ref).max(1)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


def _take(arr, rows):
    return np.stack([arr[int(r)].get() for r in rows])


def _check_norm_outputs(xn, rms, rows, xn64, r64, M):
    gx, gr = _take(xn, rows), np.array([float(rms[int(r):int(r) + 1].get()[0]) for r in rows])
    ex = np.abs(gx - xn64).max(1)
    assert (ex <= 1e-7 + 2e-6 * np.abs(xn64).max(1)).all(), float(ex.max())
    assert (np.abs(gr - r64) <= 2e-6 * r64).all(), float((np.abs(gr - r64) / r64).max())
    assert abs(float(rms[R_ZERO:R_ZERO + 1].get()[0]) - np.sqrt(np.float32(EPS))) <= 2e-6 * np.sqrt(EPS)
    assert np.isnan(xn[M - 1].get()).all() and np.isnan(rms[M - 1:M].get()).all()
    assert (xn[M:].get() == CANARY).all() and (rms[M:].get() == CANARY).all()


def _same(a, b, M):
    """bit-identical on every row but the NaN row (the last)."""
    return float((a[:M - 1] != b[:M - 1]).sum().get()) == 0.0


def _tables(L, hd):
    inv = 1.0 / (10000 ** (np.arange(0, hd, 2)[: hd // 2] / hd))
    fr = np.outer(np.arange(L), inv)
    return np.cos(fr).astype(np.float32), np.sin(fr).astype(np.float32)


def _rope64(y, cos, sin, pos, hd):
    n, C = y.shape
    yh = y.reshape(n, C // hd, hd // 2, 2)
    c, s = cos[pos][:, None, :].astype(np.float64), sin[pos][:, None, :].astype(np.float64)
    out = np.empty_like(yh)
    out[..., 0] = yh[..., 0] * c - yh[..., 1] * s
    out[..., 1] = yh[..., 0] * s + yh[..., 1] * c
    return out.reshape(n, C)


@pytest.mark.parametrize("M,F,up_first,norm", [(16384, 768, False, True), (16384 + 37, 768, True, True), (65536, 768, False, True),
                                               (16384, 192, True, True), (16384 + 37, 192, False, False), (65536, 192, False, True),
                                               (16384, 768, True, False)])
def test_gate_up_swiglu_at_fp32_accuracy(hip, M, F, up_first, norm):
    L, hp = _lib_hp()
    rng = np.random.default_rng(M + F)
    x = _x(M, rng)
    wn = rng.uniform(0.5, 1.5, K).astype(np.float32)
    wg = (0.08 * rng.standard_normal((K, F))).astype(np.float32)
    wu = (0.08 * rng.standard_normal((K, F))).astype(np.float32)
    wg[:, C_TINY] = (1e-6 * rng.standard_normal(K)).astype(np.float32)
    buf = hp.empty((2, K, F), np.float32)
    buf[1 if up_first else 0] = hp.from_numpy(wg)
    buf[0 if up_first else 1] = hp.from_numpy(wu)
    dg, stride = buf[1 if up_first else 0], (-K * F if up_first else K * F)
    xd, wnd = hp.from_numpy(x), hp.from_numpy(wn)
    rows = _rows(M)
    if norm:
        assert L.query("pdn_gateup_swiglu_norm_supported", M, F, K)
        a64, r64 = _norm64(x[rows, :K], wn)
    else:
        a64 = x[rows, :K].astype(np.float64)
    g64, u64 = a64 @ wg.astype(np.float64), a64 @ wu.astype(np.float64)
    with np.errstate(over="ignore"):                                          # (exp(3e5) = inf: silu = -0 there, as it should be)
        gu64, h64 = np.concatenate([g64, u64], 1), g64 / (1 + np.exp(-g64)) * u64

    def run():
        gu, h = hp.empty((M + 8, 2 * F), np.float32), hp.empty((M + 8, F), np.float32)
        xn, rms = hp.empty((M + 8, K), np.float32), hp.empty((M + 8,), np.float32)
        for a in (gu, h, xn, rms):
            a[...] = CANARY
        if norm:
            L.call("pdn_gateup_swiglu_norm_fwd_f32", xd._ptr, wnd._ptr, EPS, xn._ptr, rms._ptr, dg._ptr, stride, gu._ptr, h._ptr,
                   M, F, K, K + PAD, hp.stream())
        else:
            L.call("pdn_gateup_swiglu_fwd_f32", xd._ptr, dg._ptr, stride, gu._ptr, h._ptr, M, F, K, K + PAD, hp.stream())
        return gu, h, xn, rms

    _counters(L, True)
    gu, h, xn, rms = run()
    cnt = _counters(L, True)
    assert cnt[41] == 1 and cnt[2] == 1, (cnt[2], cnt[41])
    prev = L.query("pdn_gemm_rowtile_mode", 3)
    try:
        gu32, h32, xn32, rms32 = run()
    finally:
        L.query("pdn_gemm_rowtile_mode", prev)
    cnt = _counters(L, True)
    assert cnt[41] == 0 and cnt[2] == 1, (cnt[2], cnt[41])

    keep = rows != M - 1
    for name, got, got32, ref in (("gu", gu, gu32, gu64), ("h", h, h32, h64)):
        e_split, e_f32 = _worst(_take(got, rows)[keep], ref[keep]), _worst(_take(got32, rows)[keep], ref[keep])
        print(f"gate|up M={M} F={F} up_first={up_first} norm={norm}: worst row error / max |{name}|: split {e_split:.3e}, fp32 kernel {e_f32:.3e}")
        assert e_split <= 2.0 * e_f32, f"{name}: split-fp16 {e_split:.3e} against 2 x fp32 kernel {e_f32:.3e}"
    # the column of 1e-6-sized weights at ITS OWN scale: the same criterion
    rk = rows[keep & (rows != R_ZERO)]
    sel = np.isin(rows, rk)
    amax = np.abs(a64[sel]).max(1)
    c, c32 = _take(gu, rk)[:, C_TINY], _take(gu32, rk)[:, C_TINY]
    ec, ec32 = np.abs(c - g64[sel, C_TINY]) / amax, np.abs(c32 - g64[sel, C_TINY]) / amax
    assert ec.max() <= 2.0 * ec32.max(), (ec.max(), ec32.max())
    # the NaN row is NaN in every output and no other row is; the zero row is zero; nothing past M or from x's padding
    assert np.isnan(gu[M - 1].get()).all() and np.isnan(h[M - 1].get()).all()
    assert np.isfinite(_take(gu, rows[keep])).all() and np.isfinite(_take(h, rows[keep])).all() and np.isfinite(gu[M - 2].get()).all()
    assert not gu[R_ZERO].get().any() and not h[R_ZERO].get().any()
    assert (gu[M:].get() == CANARY).all() and (h[M:].get() == CANARY).all()
    assert float(np.abs(_take(gu, rows[keep & (rows != R_BIG)])).max()) < 1e20
    if norm:
        _check_norm_outputs(xn, rms, rows[keep], a64[keep], r64[keep], M)
    else:
        assert (xn.get() == CANARY).all() and (rms.get() == CANARY).all()
    # a second launch: bit-identical (fixed order, no atomics)
    gu2, h2, xn2, rms2 = run()
    assert _same(gu, gu2, M) and _same(h, h2, M) and _same(xn, xn2, M) and _same(rms, rms2, M)


@pytest.mark.parametrize("M,Lq,hd,norm", [(16384, 256, 48, True), (65536, 256, 48, True), (16384, 64, 96, True),
                                          (16384 + 64, 64, 96, True), (65536, 64, 96, False), (16384 + 64, 64, 96, False)])
def test_qkv_rope_at_fp32_accuracy(hip, M, Lq, hd, norm):
    L, hp = _lib_hp()
    rng = np.random.default_rng(M + hd)
    x = _x(M, rng)
    wn = rng.uniform(0.5, 1.5, K).astype(np.float32)
    ws = [(0.08 * rng.standard_normal((K, D))).astype(np.float32) for _ in range(3)]
    ws[2][:, C_TINY] = (1e-6 * rng.standard_normal(K)).astype(np.float32)      # (in v: RoPE would mix it with its neighbour)
    buf = hp.empty((3, K, D), np.float32)
    for i in range(3):
        buf[i] = hp.from_numpy(ws[i])
    cos, sin = _tables(Lq, hd)
    tab = hp.empty((Lq, hd, 2), np.float32)
    cd, sd, xd, wnd = hp.from_numpy(cos), hp.from_numpy(sin), hp.from_numpy(x), hp.from_numpy(wn)
    L.call("pdn_rope_table_f32", cd._ptr, sd._ptr, tab._ptr, Lq, hd, hp.stream())
    rows = _rows(M)
    if norm:
        assert L.query("pdn_qkv_rope_norm_supported", M, D, K, Lq, hd)
        a64, r64 = _norm64(x[rows, :K], wn)
    else:
        assert L.query("pdn_qkv_rope_supported", M, D, K, Lq, hd)
        a64 = x[rows, :K].astype(np.float64)
    pos = rows % Lq
    v64 = a64 @ ws[2].astype(np.float64)
    ref = np.concatenate([_rope64(a64 @ ws[0].astype(np.float64), cos, sin, pos, hd),
                          _rope64(a64 @ ws[1].astype(np.float64), cos, sin, pos, hd), v64], 1)

    def run():
        qkv = hp.empty((M + 8, 3 * D), np.float32)
        xn, rms = hp.empty((M + 8, K), np.float32), hp.empty((M + 8,), np.float32)
        for a in (qkv, xn, rms):
            a[...] = CANARY
        if norm:
            L.call("pdn_qkv_rope_norm_fwd_f32", xd._ptr, wnd._ptr, EPS, xn._ptr, rms._ptr, buf[0]._ptr, K * D, qkv._ptr, tab._ptr,
                   M, D, K, Lq, hd, K + PAD, hp.stream())
        else:
            L.call("pdn_qkv_rope_fwd_f32", xd._ptr, buf[0]._ptr, K * D, qkv._ptr, tab._ptr, M, D, K, Lq, hd, K + PAD, hp.stream())
        return qkv, xn, rms

    _counters(L, True)
    qkv, xn, rms = run()
    cnt = _counters(L, True)
    assert cnt[41] == 1 and cnt[4] == 1, (cnt[4], cnt[41])
    prev = L.query("pdn_gemm_rowtile_mode", 3)
    try:
        qkv32, xn32, rms32 = run()
    finally:
        L.query("pdn_gemm_rowtile_mode", prev)
    cnt = _counters(L, True)
    assert cnt[41] == 0 and cnt[4] == 1, (cnt[4], cnt[41])

    keep = rows != M - 1
    e_split, e_f32 = _worst(_take(qkv, rows)[keep], ref[keep]), _worst(_take(qkv32, rows)[keep], ref[keep])
    print(f"q|k|v M={M} L={Lq} hd={hd} norm={norm}: worst row error / max |qkv|: split {e_split:.3e}, fp32 kernel {e_f32:.3e}")
    assert e_split <= 2.0 * e_f32, f"split-fp16 {e_split:.3e} against 2 x fp32 kernel {e_f32:.3e}"
    rk = rows[keep & (rows != R_ZERO)]
    sel = np.isin(rows, rk)
    amax = np.abs(a64[sel]).max(1)
    c, c32 = _take(qkv, rk)[:, 2 * D + C_TINY], _take(qkv32, rk)[:, 2 * D + C_TINY]
    ec, ec32 = np.abs(c - v64[sel, C_TINY]) / amax, np.abs(c32 - v64[sel, C_TINY]) / amax
    assert ec.max() <= 2.0 * ec32.max(), (ec.max(), ec32.max())
    assert np.isnan(qkv[M - 1].get()).all()
    assert np.isfinite(_take(qkv, rows[keep])).all() and np.isfinite(qkv[M - 2].get()).all()
    assert not qkv[R_ZERO].get().any()
    assert (qkv[M:].get() == CANARY).all()
    assert float(np.abs(_take(qkv, rows[keep & (rows != R_BIG)])).max()) < 1e20
    if norm:
        _check_norm_outputs(xn, rms, rows[keep], a64[keep], r64[keep], M)
    else:
        assert (xn.get() == CANARY).all() and (rms.get() == CANARY).all()
    qkv2, xn2, rms2 = run()
    assert _same(qkv, qkv2, M) and _same(xn, xn2, M) and _same(rms, rms2, M)


def _step(dev, L, mode):
    """A 2-layer width-288 Llama, one loss + backward at 16384 tokens, built like `_block_step` of tests/test_fused_epilogues.py."""
    import pydynet_amd as pdn
    from pydynet_amd.core.tensor import Graph
    from pydynet_amd.llm.llama import Llama
    prev = L.query("pdn_gemm_rowtile_mode", mode)
    try:
        Graph.clear()
        np.random.seed(5)
        V, H, F, Lq, B = 64, 6, 192, 64, 256
        model = Llama(V, D, H, F, Lq, B, 2, np.float32)
        rng = np.random.default_rng(6)
        model.tok_embedding.weight.data[...] = (0.5 * rng.standard_normal((V, D))).astype(np.float32)
        for n, p_ in model.named_parameters():
            if n.endswith("norm.weight"):
                p_.data[...] = rng.uniform(0.5, 1.5, p_.shape).astype(np.float32)
        model.to(dev)
        ids, tgt = rng.integers(0, V, (B, Lq)), rng.integers(0, V, (B, Lq))
        _counters(L, True)
        loss = model.loss(ids, tgt)
        loss.backward()
        cnt = _counters(L, True)
        host = lambda t: t.numpy() if isinstance(t, pdn.Tensor) else (t if isinstance(t, np.ndarray) else t.get())
        grads = {n: host(p_.grad) for n, p_ in model.named_parameters() if p_.requires_grad and p_.grad is not None}
        return float(host(loss)), grads, cnt
    finally:
        L.query("pdn_gemm_rowtile_mode", prev)
        Graph.clear()


def test_training_step_with_the_split_on_and_off(hip):
    from tests.test_fused_epilogues import close, RT
    L, _ = _lib_hp()
    l1, g1, c1 = _step("hip:0", L, 1)
    l0, g0, c0 = _step("hip:0", L, 3)
    assert c1[41] == 4 and c1[2] == 2 and c1[4] == 2, (c1[2], c1[4], c1[41])     # both projections of both layers
    assert c0[41] == 0 and c0[2] == 2 and c0[4] == 2, (c0[2], c0[4], c0[41])
    print(f"step: loss split {l1:.7f}, fp32 kernels {l0:.7f}")
    assert abs(l1 - l0) <= RT * abs(l0), (l1, l0)
    assert g1.keys() == g0.keys() and len(g1) >= 20
    for n in g0:
        close(g1[n], g0[n], f"grad {n}")
