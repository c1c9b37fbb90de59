"""The streaming row kernels of csrc/fused.hip (softmax, RMSNorm, cross entropy, embedding, RoPE, SwiGLU, Adam, the
device-scalar scale) and the reductions of csrc/reduce.hip, called through the C ABI at every variant their dispatch code
can choose -- each template instantiation, the block / scalar fallbacks behind a misaligned base, both sides of every
threshold, one shape past each grid cap -- against the float64 statements of tests/row_kernels_ref.py.

Every check is a `check_*(dev)` registered through `device_variants`: it runs on the MI355X under `-m gpu` and on the NumPy
emulation of the C ABI otherwise.  Each docstring names the kernels its shapes were chosen to reach.

Criteria (tests/test_kernels_gpu.py): bit-exact for copies, index work and masked zeros; rtol 2e-5 / atol 2e-6 against
float64 for streams; 1e-4 of the reference's largest entry where the summation order differs.  Inputs with a large common
offset or a wide spread lose more than that to fp32 in the statement itself, whoever evaluates it: there the kernel's
error against float64 is held to 4 x the error of the same statement evaluated by NumPy in float32 (the factor is for a
different summation order), and both are printed (pairs measured on an MI355X: profiles/row_kernels_gpu_tests.txt)."""
import ctypes
import math

import numpy as np
import pytest

from tests import row_kernels_ref as ref
from tests.conftest import device_variants

F32, F64 = np.float32, np.float64
RT, AT = 2e-5, 2e-6                      # the stream tolerance of tests/test_kernels_gpu.py
EINVAL, EWORKSPACE = -1, -3
CNT_CE_SMALL = 18                        # PDN_CNT_CE_SMALL (csrc/common.h)


def _env(dev):
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.cuda import Device
    return hp, _lib.lib(), Device(dev)


def _emulated(L):
    return type(L).__name__ == "EmulatedLib"


class Buf:
    """A host array on the device with four guard elements on either side of it; `off` elements (0..3) of the leading
    guard are skipped, which puts a float32 base `4 * off` bytes off the 16-byte grid.  get() checks the guards."""

    def __init__(self, hp, a, off=0, dtype=F32):
        a = np.asarray(a, dtype)
        self.shape, self.n, self.lead = a.shape, a.size, 4 + off
        host = np.zeros(self.n + 8 + off, dtype)
        host[self.lead:self.lead + self.n] = a.ravel()
        self.dev = hp.from_numpy(host)
        self.ptr = self.dev._ptr + self.lead * host.itemsize

    def get(self):
        h = self.dev.get()
        assert not h[:self.lead].any() and not h[self.lead + self.n:].any(), "a kernel wrote outside its buffer"
        return h[self.lead:self.lead + self.n].reshape(self.shape)


def _nan(shape):
    return np.full(shape, np.nan, F32)


def _close(got, want, what):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(np.abs(got - want) <= AT + RT * np.abs(want))
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.abs(got - want), 0))), got.shape)
        raise AssertionError((what, "elements off", int(bad.sum()), "worst at", i, float(got[i]), float(want[i])))


def _sumtol(got, want, what):
    """Where the summation order differs: 1e-4 of the reference's largest entry."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= 1e-4 * scale, (what, err, scale)


def _inherent(got, same_in_f32, want, what):
    """The kernel's error against float64 within 4 x the error of the same statement in NumPy float32."""
    got, f32, want = (np.asarray(a, F64) for a in (got, same_in_f32, want))
    assert got.shape == want.shape == f32.shape and np.isfinite(want).all() and np.isfinite(got).all(), what
    err, own = float(np.abs(got - want).max()), float(np.abs(f32 - want).max())
    print(f"{what}: kernel err {err:.3e}, float32 statement err {own:.3e}, of {float(np.abs(want).max()):.3e}")
    assert err <= 4.0 * own, (what, err, own)


def _refused(L, code, name, *args):
    """The entry refuses on the host: the status code, and (real library) pdn_last_error names the entry."""
    from pydynet_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError) as e:
        L.call(name, *args)
    assert e.value.code == code, (name, e.value.code)
    if not _emulated(L):
        assert name in L._last_error().decode(), (name, L._last_error())


def _flag_raised_then_cleared(hp):
    with pytest.raises(IndexError):
        hp.check_index_errors()
    hp.check_index_errors()                              # cleared by the raise


# =====================================================================================================================
# softmax
# =====================================================================================================================
DIVISORS = (1.0, float(F32(math.sqrt(48.0))), 8.0)
WAVE_COLS = (4, 252, 256, 260, 512, 516, 768, 772, 1020, 1024)      # VPL 1 | 1 1 2 | 2 3 | 3 4 | 4 4: full / partial last
BLOCK_COLS = (1, 3, 10, 77, 1026, 1028, 4099)


def _softmax_case(hp, L, rng, rows, cols, divisor=1.0, cl=0, sp=0, off=0, x=None, inherent=False):
    what = ("softmax", rows, cols, round(divisor, 3), cl, sp, off)
    if x is None:
        x = (3.0 * rng.standard_normal((rows, cols))).astype(F32)
    X, Y = Buf(hp, x, off), Buf(hp, _nan(x.shape), off)
    L.call("pdn_softmax_fwd_f32", X.ptr, Y.ptr, rows, cols, divisor, cl, sp, hp.stream())
    y, want = Y.get(), ref.softmax_fwd(x, divisor, cl, sp)
    assert np.isfinite(want).all(), what
    assert np.array_equal(X.get(), x), what + ("input changed",)
    assert np.all(y[~ref.causal_keep(rows, cols, cl, sp)] == 0.0), what + ("masked entries are not exactly 0",)
    if inherent:
        _inherent(y, ref.softmax_fwd(x, divisor, cl, sp, dtype=F32), want, what)
    else:
        _close(y, want, what)
    _close(y.sum(-1, dtype=F64), np.ones(rows), what + ("row sums",))
    X2 = Buf(hp, x, off)                                                        # in place (core/fused/attn.py)
    L.call("pdn_softmax_fwd_f32", X2.ptr, X2.ptr, rows, cols, divisor, cl, sp, hp.stream())
    assert np.array_equal(X2.get(), y), what + ("in place differs",)
    dy = rng.standard_normal((rows, cols)).astype(F32)
    DY, DX = Buf(hp, dy, off), Buf(hp, _nan(x.shape), off)
    L.call("pdn_softmax_bwd_f32", Y.ptr, DY.ptr, DX.ptr, rows, cols, divisor, hp.stream())
    dx = DX.get()
    _close(dx, ref.softmax_bwd(y, dy, divisor), what + ("dx",))
    L.call("pdn_softmax_bwd_f32", Y.ptr, DY.ptr, DY.ptr, rows, cols, divisor, hp.stream())
    assert np.array_equal(DY.get(), dx), what + ("dx in place differs",)


def check_softmax_wave_every_vpl(dev):
    """softmax_fwd_wave_kernel / softmax_bwd_wave_kernel <1 | 2 | 3 | 4> (cols % 4 == 0, <= 1024, 16-byte bases): each VPL
    with a full and a partial last vector, 1 and 5 rows (one workgroup holds 4), the three divisors, forward and backward,
    out of place and in place."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(201)
    with device:
        for cols in WAVE_COLS:
            for rows in (1, 5):
                for d in DIVISORS:
                    _softmax_case(hp, L, rng, rows, cols, d)


def check_softmax_block_kernel(dev):
    """softmax_fwd_block_kernel / softmax_bwd_block_kernel: cols % 4 != 0, cols > 1024 (one and several trips of the 256
    threads), and wave-sized rows whose base is 4 bytes off the 16-byte grid (the misaligned-base fallback)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(202)
    with device:
        for cols in BLOCK_COLS:
            for rows in (1, 5):
                for d in DIVISORS:
                    _softmax_case(hp, L, rng, rows, cols, d)
        for cols in (256, 1024):
            for rows in (1, 5):
                _softmax_case(hp, L, rng, rows, cols, DIVISORS[1], off=1)


def check_softmax_past_the_grid_caps(dev):
    """wave_grid covers 16384 rows per pass (4096 workgroups x 4 waves): 16390 x 8 turns the row loop of the wave
    kernels; the block kernels take 4096 rows per pass: 4100 x 10."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(203)
    with device:
        _softmax_case(hp, L, rng, 16390, 8, DIVISORS[1])
        _softmax_case(hp, L, rng, 4100, 10, DIVISORS[1])


def check_softmax_causal_and_start_pos(dev):
    """The causal prologue (limit = row % causal_L + start_pos) with start_pos 0 and 5: the wave kernel at 72 columns
    (the limit falls inside a float4 at every phase), the block kernel at 64 + start_pos columns (64: behind a misaligned
    base) and at cols % 4 != 0; 131 rows, so row % causal_L wraps twice.  Masked entries are exactly 0."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(204)
    with device:
        for sp in (0, 5):
            _softmax_case(hp, L, rng, 131, 72, DIVISORS[1], cl=64, sp=sp)                  # wave
            _softmax_case(hp, L, rng, 131, 64 + sp, DIVISORS[1], cl=64, sp=sp, off=1)      # block
            _softmax_case(hp, L, rng, 131, 67 + sp, DIVISORS[1], cl=64, sp=sp)             # block, cols % 4 != 0


def check_softmax_large_offset_and_spread(dev):
    """A common offset of +1e4 (the maximum shift has to be taken before the exponential) and a row spread over +-300
    (entries underflow), on the wave kernel (256 columns) and the block kernel (77): against float64 within 4 x the
    error of the float32 statement."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(205)
    with device:
        for cols in (256, 77):
            x = (3.0 * rng.standard_normal((5, cols)) + 1e4).astype(F32)
            _softmax_case(hp, L, rng, 5, cols, x=x, inherent=True)
            x = (3.0 * rng.standard_normal((5, cols))).astype(F32)
            x[2] = rng.permutation(np.linspace(-300.0, 300.0, cols)).astype(F32)
            _softmax_case(hp, L, rng, 5, cols, x=x, inherent=True)


# =====================================================================================================================
# RMSNorm
# =====================================================================================================================
RMS_COLS = (4, 64, 256, 260, 512, 768, 1020, 1024, 1028, 1536, 2044, 2048)     # VPL 1 1 1 2 2 3 4 4 5 6 8 8


def _rms_ws(hp, L, rows, cols):
    nbytes = L.query("pdn_rmsnorm_bwd_workspace_bytes", rows, cols)
    return Buf(hp, np.zeros(nbytes // 4, F32)), nbytes


def _rmsnorm_case(hp, L, rng, rows, cols, eps=1e-6):
    what = ("rmsnorm", rows, cols, eps)
    x = rng.standard_normal((rows, cols)).astype(F32) * 2
    w = (1.0 + 0.3 * rng.standard_normal(cols)).astype(F32)
    dy, res = rng.standard_normal((rows, cols)).astype(F32), rng.standard_normal((rows, cols)).astype(F32)
    X, W, DY, RES = Buf(hp, x), Buf(hp, w), Buf(hp, dy), Buf(hp, res)
    Y, RMS, Y0 = Buf(hp, _nan(x.shape)), Buf(hp, _nan(rows)), Buf(hp, _nan(x.shape))
    L.call("pdn_rmsnorm_fwd_f32", X.ptr, W.ptr, Y.ptr, RMS.ptr, rows, cols, eps, hp.stream())
    L.call("pdn_rmsnorm_fwd_f32", X.ptr, W.ptr, Y0.ptr, None, rows, cols, eps, hp.stream())     # rms = NULL (decode)
    y, rms = Y.get(), RMS.get()
    y_ref, rms_ref = ref.rmsnorm_fwd(x, w, eps)
    _close(y, y_ref, what + ("y",))
    _close(rms, rms_ref, what + ("rms",))
    assert np.array_equal(Y0.get(), y), what + ("rms = NULL changes y",)
    WS, wsb = _rms_ws(hp, L, rows, cols)
    dx_ref, dw_ref = ref.rmsnorm_bwd(x, w, rms, dy)
    dxr_ref, _ = ref.rmsnorm_bwd(x, w, rms, dy, res)
    # accumulate_dw = 0 over garbage
    DX, DW = Buf(hp, _nan(x.shape)), Buf(hp, _nan(cols))
    L.call("pdn_rmsnorm_bwd_f32", X.ptr, W.ptr, RMS.ptr, DY.ptr, None, DX.ptr, DW.ptr, 0, rows, cols, WS.ptr, wsb, hp.stream())
    _close(DX.get(), dx_ref, what + ("dx",))
    _sumtol(DW.get(), dw_ref, what + ("dw",))
    # accumulate_dw = 1 over non-zero values, with the residual
    dw0 = rng.standard_normal(cols).astype(F32)
    DX, DW = Buf(hp, _nan(x.shape)), Buf(hp, dw0)
    L.call("pdn_rmsnorm_bwd_f32", X.ptr, W.ptr, RMS.ptr, DY.ptr, RES.ptr, DX.ptr, DW.ptr, 1, rows, cols, WS.ptr, wsb, hp.stream())
    _close(DX.get(), dxr_ref, what + ("dx + residual",))
    _sumtol(DW.get(), dw0.astype(F64) + dw_ref, what + ("dw accumulated",))
    # dw = NULL (no workspace either) with the residual
    DX = Buf(hp, _nan(x.shape))
    L.call("pdn_rmsnorm_bwd_f32", X.ptr, W.ptr, RMS.ptr, DY.ptr, RES.ptr, DX.ptr, None, 0, rows, cols, None, 0, hp.stream())
    _close(DX.get(), dxr_ref, what + ("dx + residual, dw = NULL",))
    for b in (X, W, DY, RES):
        b.get()


def check_rmsnorm_every_vpl(dev):
    """rmsnorm_fwd_kernel / rmsnorm_bwd_kernel <1..8>: column counts on both sides of every 256-column step, with 1, 3
    and 17 rows (17: a second workgroup, whose dw partial colsum_partials_kernel adds); rms = NULL forward; dw written over
    garbage, accumulated over values, and absent, with and without dx_residual."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(211)
    with device:
        for cols in RMS_COLS:
            for rows in (1, 3, 17):
                _rmsnorm_case(hp, L, rng, rows, cols)
        _rmsnorm_case(hp, L, rng, 3, 260, eps=10.0)                                # an eps that dominates mean(x^2)


def check_rmsnorm_past_the_caps(dev):
    """16400 x 64: past the 16384 rows one pass of the forward grid covers, and past the 1024 workgroups (16 rows each)
    of the backward, whose waves then walk several rows each and whose partials fill the whole workspace."""
    hp, L, device = _env(dev)
    with device:
        _rmsnorm_case(hp, L, np.random.default_rng(212), 16400, 64)


def check_rmsnorm_refusals(dev):
    """cols > 2048, cols % 4 != 0, a workspace one byte short and operands off the 16-byte grid are refused on the host
    (status code, pdn_last_error) by pdn_rmsnorm_fwd_f32 and pdn_rmsnorm_bwd_f32: nothing is written."""
    hp, L, device = _env(dev)
    rows = 3
    with device:
        for cols, off, short in ((2052, 0, 0), (6, 0, 0), (64, 1, 0), (64, 0, 1)):
            n = rows * cols
            X, W, DY = Buf(hp, np.ones(n, F32), off), Buf(hp, np.ones(cols, F32)), Buf(hp, np.ones(n, F32))
            Y, RMS, DX, DW = Buf(hp, _nan(n)), Buf(hp, np.ones(rows, F32)), Buf(hp, _nan(n)), Buf(hp, _nan(cols))
            WS, wsb = _rms_ws(hp, L, rows, cols)
            st = hp.stream()
            if not short:
                _refused(L, EINVAL, "pdn_rmsnorm_fwd_f32", X.ptr, W.ptr, Y.ptr, RMS.ptr, rows, cols, 1e-6, st)
            _refused(L, EWORKSPACE if short else EINVAL, "pdn_rmsnorm_bwd_f32", X.ptr, W.ptr, RMS.ptr, DY.ptr, None, DX.ptr,
                     DW.ptr, 0, rows, cols, WS.ptr, wsb - short, st)
            if off:                                          # each float4 operand of the backward on its own
                X0 = Buf(hp, np.ones(n, F32))
                for args in ((X0.ptr, W.ptr + 4, RMS.ptr, DY.ptr, None, DX.ptr), (X0.ptr, W.ptr, RMS.ptr, DY.ptr + 4, None, DX.ptr),
                             (X0.ptr, W.ptr, RMS.ptr, DY.ptr, X.ptr, DX.ptr), (X0.ptr, W.ptr, RMS.ptr, DY.ptr, None, DX.ptr + 4)):
                    _refused(L, EINVAL, "pdn_rmsnorm_bwd_f32", *args, DW.ptr, 0, rows, cols, WS.ptr, wsb, st)
            for out in (Y, DX, DW):
                assert np.isnan(out.get()).all(), ("written by a refused call", cols, off, short)


# =====================================================================================================================
# cross entropy
# =====================================================================================================================
CE_REG = ((258, 4096), (300, 4100), (258, 32768), (3, 8192))          # ce_fwd_bwd_reg_kernel; > 256 rows: the prefetch runs
CE_SMALL = ((1024, 10), (1030, 16), (1025, 17), (1024, 32))           # ce_small_kernel<16 | 32>
CE_GENERIC = ((1023, 10), (40, 33), (37, 4097), (520, 4098), (20, 32772), (9, 50001))   # ce_fwd_kernel / ce_fwd_bwd_kernel


def _counter(L, slot):
    out = (ctypes.c_int64 * 64)()
    L.call("pdn_kernel_counters", out, 64, 0)
    return int(out[slot])


def _ce_inputs(rng, rows, V):
    x = (2.0 * rng.standard_normal((rows, V))).astype(F32)
    off_rows = [0] if rows < 8 else [0, 5, 6, 7]
    x[off_rows] += F32(3e4)                                              # a common offset: the maximum shift must work
    x[1] = rng.permutation(np.linspace(-200.0, 200.0, V)).astype(F32)    # a row spread over +-200
    x[2, [1, 5, V // 2, V - 3]] = -np.inf                                # -inf away from the target: gradient exactly 0
    t = rng.integers(0, V, rows)
    special = (0, V - 1, -1, -V, V - 2)              # column 0, the last column / last partial vector, negative targets
    t[:min(rows, 5)] = special[:min(rows, 5)]
    plain = np.setdiff1d(np.arange(rows), off_rows + [1])
    return x, t.astype(np.int64), off_rows, plain


def _ce_compare(got, want, f32, off_rows, plain, what):
    _close(got[plain], want[plain], what)
    _inherent(got[off_rows], f32[off_rows], want[off_rows], what + ("offset +3e4",))
    _inherent(got[1:2], f32[1:2], want[1:2], what + ("spread +-200",))


def _ce_case(hp, L, rng, rows, V, kind):
    what = ("ce", kind, rows, V)
    x, t, off_rows, plain = _ce_inputs(rng, rows, V)
    gscale, st = 0.37, hp.stream()
    want, f32 = ref.cross_entropy(x, t, gscale, mean=True), ref.cross_entropy(x, t, gscale, mean=True, dtype=F32)
    assert all(np.isfinite(a).all() for a in want), what
    X, T = Buf(hp, x), Buf(hp, t, dtype=np.int64)
    err = hp.err_flag_ptr()
    new = lambda *shape: Buf(hp, _nan(shape))

    # forward only (mean): ce_fwd_kernel, or the register kernel without the write
    LR, LSE, OUT = new(rows), new(rows), new(1)
    L.call("pdn_cross_entropy_fwd_f32", X.ptr, T.ptr, rows, V, 1, LR.ptr, LSE.ptr, OUT.ptr, err, st)
    loss_row, lse = LR.get(), LSE.get()
    _ce_compare(loss_row, want[0], f32[0], off_rows, plain, what + ("fwd loss_row",))
    _ce_compare(lse, want[1], f32[1], off_rows, plain, what + ("fwd lse_row",))
    _close(OUT.get()[0], loss_row.astype(F64).mean(), what + ("fwd loss (mean)",))

    # forward + backward in one pass (sum, gscale != 1 / rows)
    c0 = _counter(L, CNT_CE_SMALL)
    LR2, LSE2, OUT2, DL = new(rows), new(rows), new(1), new(rows, V)
    L.call("pdn_cross_entropy_fwd_bwd_f32", X.ptr, T.ptr, rows, V, 0, gscale, LR2.ptr, LSE2.ptr, OUT2.ptr, DL.ptr, None, None,
           0, err, st)
    assert _counter(L, CNT_CE_SMALL) - c0 == (1 if kind == "small" else 0), what + ("PDN_CNT_CE_SMALL",)
    d, lr2 = DL.get(), LR2.get()
    _ce_compare(lr2, want[0], f32[0], off_rows, plain, what + ("fwd_bwd loss_row",))
    _ce_compare(LSE2.get(), want[1], f32[1], off_rows, plain, what + ("fwd_bwd lse_row",))
    _close(OUT2.get()[0], LR2.get().astype(F64).sum(), what + ("fwd_bwd loss (sum)",))
    _ce_compare(d, want[3], f32[3], off_rows, plain, what + ("dlogits",))
    assert np.all(d[2, [1, 5, V // 2, V - 3]] == 0.0), what + ("gradient at -inf",)
    if kind == "reg":                                  # the fused column sums (the bias gradient of the vocabulary layer)
        nbytes = L.query("pdn_cross_entropy_colsum_workspace_bytes", rows, V)
        assert nbytes > 0, what
        WS, CS, DL2 = Buf(hp, np.zeros(nbytes // 4, F32)), new(V), new(rows, V)
        L.call("pdn_cross_entropy_fwd_bwd_f32", X.ptr, T.ptr, rows, V, 0, gscale, LR2.ptr, LSE2.ptr, OUT2.ptr, DL2.ptr, CS.ptr,
               WS.ptr, nbytes, err, st)
        assert np.array_equal(DL2.get(), d), what + ("dlogits with column sums",)
        _sumtol(CS.get(), d.astype(F64).sum(0), what + ("dlogits_colsum",))
    else:
        assert L.query("pdn_cross_entropy_colsum_workspace_bytes", rows, V) == 0, what

    # backward from the stored lse, upstream 0.5 on the device; then with dlogits aliasing logits
    UP, DB = Buf(hp, np.array([0.5], F32)), new(rows, V)
    L.call("pdn_cross_entropy_bwd_f32", X.ptr, T.ptr, LSE.ptr, UP.ptr, gscale, DB.ptr, rows, V, st)
    db = DB.get()
    _ce_compare(db, 0.5 * want[3], F32(0.5) * f32[3], off_rows, plain, what + ("bwd dlogits",))
    assert np.all(db[2, [1, 5, V // 2, V - 3]] == 0.0), what + ("bwd gradient at -inf",)
    XA = Buf(hp, x)
    L.call("pdn_cross_entropy_bwd_f32", XA.ptr, T.ptr, LSE.ptr, UP.ptr, gscale, XA.ptr, rows, V, st)
    assert np.array_equal(XA.get(), db), what + ("bwd in place differs",)

    # the loss from row statistics that exist already (non-negative targets: see check_cross_entropy_from_lse_targets)
    TW, LR3, OUT3 = Buf(hp, ref.wrap(t, V), dtype=np.int64), new(rows), new(1)
    for mean in (0, 1):
        L.call("pdn_cross_entropy_from_lse_f32", X.ptr, V, LSE.ptr, TW.ptr, rows, V, mean, LR3.ptr, OUT3.ptr, err, st)
        lr3 = LR3.get()
        assert np.array_equal(lr3, loss_row), what + ("from_lse loss_row",)
        _close(OUT3.get()[0], lr3.astype(F64).mean() if mean else lr3.astype(F64).sum(), what + ("from_lse loss", mean))
    hp.check_index_errors()                                                # nothing above raised the flag

    # one target outside [-V, V): the flag goes up, the other rows are unaffected, the flag is cleared by the check
    tb = t.copy()
    tb[rows - 1] = V
    TB = Buf(hp, tb, dtype=np.int64)
    L.call("pdn_cross_entropy_fwd_bwd_f32", X.ptr, TB.ptr, rows, V, 0, gscale, LR2.ptr, LSE2.ptr, OUT2.ptr, DL.ptr, None, None,
           0, err, st)
    assert np.array_equal(DL.get()[:-1], d[:-1]) and np.array_equal(LR2.get()[:-1], lr2[:-1]), what + ("rows beside a bad target",)
    _flag_raised_then_cleared(hp)
    L.call("pdn_cross_entropy_fwd_f32", X.ptr, TB.ptr, rows, V, 1, LR.ptr, LSE.ptr, OUT.ptr, err, st)
    assert np.array_equal(LR.get()[:-1], loss_row[:-1]) and np.array_equal(LSE.get(), lse), what + ("fwd beside a bad target",)
    _flag_raised_then_cleared(hp)
    assert np.array_equal(X.get(), x) and np.array_equal(T.get(), t), what + ("inputs changed",)


def check_cross_entropy_register_kernel(dev):
    """ce_fwd_bwd_reg_kernel <COLSUM, WRITE> (4096 <= V <= 32768, V % 4 == 0): both ends of the range, V = 4100 (a last
    float4 that only some threads hold), 258 and 300 rows (more than the 256 workgroups: the prefetch of the next row
    runs), 3 rows; with and without the fused column sums."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(221)
    with device:
        for rows, V in CE_REG:
            _ce_case(hp, L, rng, rows, V, "reg")


def check_cross_entropy_small_vocabulary_kernel(dev):
    """ce_small_kernel<16> (V <= 16) and <32> (V <= 32) from 1024 rows on, one thread per row: both templates at their
    largest V and below, full and partial last workgroups; PDN_CNT_CE_SMALL moves once per fused call."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(222)
    with device:
        for rows, V in CE_SMALL:
            _ce_case(hp, L, rng, rows, V, "small")


def check_cross_entropy_generic_kernel(dev):
    """ce_fwd_kernel / ce_fwd_bwd_kernel / ce_bwd_kernel: 1023 x 10 (one row short of ce_small), V = 33 (one class past
    it), V >= 4096 with V % 4 != 0 (1024 threads; odd V: every other row is off the 16-byte grid and takes the scalar
    loop), 520 rows (past the 512 workgroups of the wide grid), V > 32768 (past the register kernel)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(223)
    with device:
        for rows, V in CE_GENERIC:
            _ce_case(hp, L, rng, rows, V, "generic")


def check_cross_entropy_from_lse_targets(dev):
    """ce_rows_from_lse_kernel reads logits with a row stride and, unlike its siblings, reports a NEGATIVE target as an
    error (include/pdn_hip.h: the GEMMs that form its gradient clamp their targets): the flag goes up for -1 and for V,
    the other rows are unaffected."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(224)
    rows, V, ldl = 300, 50, 56
    z = rng.standard_normal((rows, ldl)).astype(F32)
    lse = rng.standard_normal(rows).astype(F32)
    t = rng.integers(0, V, rows).astype(np.int64)
    t[:2] = (0, V - 1)
    want = lse - z[np.arange(rows), t]                                         # one float32 subtraction: exact statement
    with device:
        Z, LSE, LR, OUT = Buf(hp, z), Buf(hp, lse), Buf(hp, _nan(rows)), Buf(hp, _nan(1))
        for bad in (None, -1, V):
            tb = t.copy()
            if bad is not None:
                tb[7] = bad
            T = Buf(hp, tb, dtype=np.int64)
            L.call("pdn_cross_entropy_from_lse_f32", Z.ptr, ldl, LSE.ptr, T.ptr, rows, V, 0, LR.ptr, OUT.ptr, hp.err_flag_ptr(),
                   hp.stream())
            got = LR.get()
            keep = np.arange(rows) != (7 if bad is not None else -1)
            assert np.array_equal(got[keep], want[keep]), bad
            if bad is None:
                hp.check_index_errors()
                _close(OUT.get()[0], want.astype(F64).sum(), "from_lse sum")
            else:
                _flag_raised_then_cleared(hp)


# =====================================================================================================================
# embedding, take / put columns
# =====================================================================================================================
def _ids(rng, n, V):
    ids = rng.integers(-V, V, n).astype(np.int64)                              # negative ids wrap
    if n > 65535:                                                              # first and last occurrence in different passes
        ids[0], ids[65535 + 5], ids[1], ids[n - 1] = 7, 7, -3, V - 3
    return ids


def _gather_case(hp, L, rng, n, D, V):
    what = ("gather", n, D, V)
    full = rng.standard_normal((V, D + 5)).astype(F32)
    ids = _ids(rng, n, V)
    FULL, IDS, OUT = Buf(hp, full), Buf(hp, ids, dtype=np.int64), Buf(hp, _nan((n, D)))
    L.call("pdn_embedding_gather_f32", FULL.ptr + 8, V, D, D + 5, IDS.ptr, n, OUT.ptr, hp.err_flag_ptr(), hp.stream())
    assert np.array_equal(OUT.get(), full[:, 2:2 + D][ids]), what            # a column slice: w_row_stride > D
    hp.check_index_errors()
    bad = ids.copy()
    bad[n // 2] = V
    bad[0] = -V - 1
    IDS, OUT = Buf(hp, bad, dtype=np.int64), Buf(hp, _nan((n, D)))
    L.call("pdn_embedding_gather_f32", FULL.ptr + 8, V, D, D + 5, IDS.ptr, n, OUT.ptr, hp.err_flag_ptr(), hp.stream())
    got, ok = OUT.get(), (bad >= -V) & (bad < V)
    assert np.isnan(got[~ok]).all() and np.array_equal(got[ok], full[:, 2:2 + D][bad[ok]]), what + ("bad id",)
    _flag_raised_then_cleared(hp)


def _scatter_case(hp, L, rng, n, D, V):
    what = ("scatter", n, D, V)
    g = rng.standard_normal((n, D)).astype(F32)
    ids = _ids(rng, n, V)
    if n > 4:
        ids[3] = V + 2                                                         # outside the table: skipped
    dw0 = rng.standard_normal((V, D)).astype(F32)
    owner = rng.integers(1, 3, V).astype(F32)                                  # two tags
    G, IDS, OWN = Buf(hp, g), Buf(hp, ids, dtype=np.int64), Buf(hp, owner)
    nbytes = L.query("pdn_embedding_scatter_workspace_bytes", V)
    WS = Buf(hp, np.zeros(nbytes // 4, np.int32), dtype=np.int32)
    for mode in (0, 1, 2):
        for own, tag in ((None, 0.0), (OWN, 1.0), (OWN, 2.0)):
            if own is not None and mode == 2:
                continue
            DW = Buf(hp, dw0)
            L.call("pdn_embedding_scatter_f32", G.ptr, IDS.ptr, n, DW.ptr, V, D, mode, own.ptr if own else None, tag,
                   None if mode == 2 else WS.ptr, 0 if mode == 2 else nbytes, hp.stream())
            got = DW.get()
            if mode == 2:                                                      # atomic adds: any order
                _sumtol(got, ref.scatter(dw0.astype(F64), g, ids, 2), what + (mode,))
                continue
            want = ref.scatter(dw0, g, ids, mode, owner if own else None, tag)
            assert np.array_equal(got, want), what + (mode, tag)
            if own:                                                            # rows of the other tag: bit for bit untouched
                assert np.array_equal(got[owner != tag], dw0[owner != tag]), what + (mode, tag, "other owner")
    assert np.array_equal(G.get(), g) and np.array_equal(IDS.get(), ids)


def check_embedding_gather_and_scatter(dev):
    """gather_rows_kernel (64 / 128 / 256 threads by D; a column-sliced table; negative and out-of-range ids) and
    last_occurrence_kernel + scatter_rows_kernel in mode 0 (assign the last occurrence), 1 (accumulate it) and 2 (atomic
    add), with and without the row_owner filter: D below, off and above the 64-lane grid, 1 and 300 rows."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(231)
    with device:
        for D in (8, 100, 130, 288):
            for n in (1, 300):
                _gather_case(hp, L, rng, n, D, 50)
                _scatter_case(hp, L, rng, n, D, 50)


def check_embedding_past_the_grid(dev):
    """65536 + 37 rows of D = 8: past the 65535 workgroups of gather_rows_kernel / scatter_rows_kernel, whose row loops
    turn; every id repeats across the two passes, and the last occurrence alone must land in modes 0 and 1."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(232)
    with device:
        _gather_case(hp, L, rng, 65536 + 37, 8, 500)
        _scatter_case(hp, L, rng, 65536 + 37, 8, 500)


def check_take_and_put_cols(dev):
    """take_cols_kernel / put_cols_kernel: one column per row through a row stride, negative indices, one index outside
    (flag raised, nothing written for that row); 300 rows, two workgroups."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(233)
    n, C, rs = 300, 37, 41
    x = rng.standard_normal((n, rs)).astype(F32)
    idx = rng.integers(-C, C, n).astype(np.int64)
    idx[:2] = (-C, C - 1)
    g = rng.standard_normal(n).astype(F32)
    with device:
        X, G = Buf(hp, x), Buf(hp, g)
        for bad in (None, C, -C - 1):
            ib = idx.copy()
            if bad is not None:
                ib[11] = bad
            ok = np.arange(n) != (11 if bad is not None else -1)
            IDX, OUT, DX = Buf(hp, ib, dtype=np.int64), Buf(hp, _nan(n)), Buf(hp, np.zeros((n, C), F32))
            L.call("pdn_take_cols_f32", X.ptr, n, C, rs, IDX.ptr, OUT.ptr, hp.err_flag_ptr(), hp.stream())
            L.call("pdn_put_cols_f32", G.ptr, IDX.ptr, DX.ptr, n, C, hp.stream())
            out, want_dx = OUT.get(), np.zeros((n, C), F32)
            want_dx[np.arange(n)[ok], ib[ok]] = g[ok]
            assert np.array_equal(out[ok], x[np.arange(n)[ok], ref.wrap(ib[ok], C)]) and np.isnan(out[~ok]).all(), bad
            assert np.array_equal(DX.get(), want_dx), bad
            if bad is None:
                hp.check_index_errors()
            else:
                _flag_raised_then_cleared(hp)


# =====================================================================================================================
# RoPE
# =====================================================================================================================
def _rope_case(hp, L, rng, B, Lq, heads, hd):
    what = ("rope", B, Lq, heads, hd)
    rows, D, half, st = B * Lq, heads * hd, hd // 2, hp.stream()
    ang = rng.uniform(-3.0, 3.0, (Lq, half))
    cos, sin = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
    x = rng.standard_normal((rows, heads, hd)).astype(F32)
    want = ref.rope(x, cos, sin, Lq)
    X, C, S, Y, XB = Buf(hp, x), Buf(hp, cos), Buf(hp, sin), Buf(hp, _nan(x.shape)), Buf(hp, _nan(x.shape))
    L.call("pdn_rope_f32", X.ptr, C.ptr, S.ptr, Y.ptr, rows, Lq, heads, hd, 0, st)
    _close(Y.get(), want, what + ("forward",))
    L.call("pdn_rope_f32", Y.ptr, C.ptr, S.ptr, XB.ptr, rows, Lq, heads, hd, 1, st)
    _close(XB.get(), ref.rope(Y.get(), cos, sin, Lq, -1.0), what + ("backward",))
    _close(XB.get(), x, what + ("backward inverts forward",))
    # the packed q | k | v projection (T, 3D): 2 * heads heads of q | k rotated in place, v untouched
    qkv = rng.standard_normal((rows, 3 * D)).astype(F32)
    want_qk = ref.rope(qkv[:, :2 * D].reshape(rows, 2 * heads, hd), cos, sin, Lq).reshape(rows, 2 * D)
    P = Buf(hp, qkv)
    L.call("pdn_rope_rows_f32", P.ptr, C.ptr, S.ptr, P.ptr, rows, Lq, 2 * heads, hd, 3 * D, 3 * D, 0, st)
    got = P.get()
    _close(got[:, :2 * D], want_qk, what + ("rows, in place",))
    assert np.array_equal(got[:, 2 * D:], qkv[:, 2 * D:]), what + ("v columns changed",)
    # x_row_stride != y_row_stride: from the packed buffer into a dense (T, 2D) one, and back with backward = 1
    P, Q = Buf(hp, qkv), Buf(hp, _nan((rows, 2 * D)))
    L.call("pdn_rope_rows_f32", P.ptr, C.ptr, S.ptr, Q.ptr, rows, Lq, 2 * heads, hd, 3 * D, 2 * D, 0, st)
    assert np.array_equal(Q.get(), got[:, :2 * D]), what + ("rows, strides differ",)
    L.call("pdn_rope_rows_f32", Q.ptr, C.ptr, S.ptr, P.ptr, rows, Lq, 2 * heads, hd, 2 * D, 3 * D, 1, st)
    back = P.get()
    _close(back[:, :2 * D], qkv[:, :2 * D], what + ("rows, backward inverts forward",))
    assert np.array_equal(back[:, 2 * D:], qkv[:, 2 * D:]), what + ("v columns changed (backward)",)


def check_rope_shapes(dev):
    """rope_kernel and rope_rows_kernel: head dims 2 (one pair), 48, 64, 128; 1 and 6 heads; 1 and 16 positions; 1 and 3
    sequences (row % L picks the table row); in place on a packed q | k | v buffer, between buffers of different row
    strides, and backward = 1 as the inverse."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(241)
    with device:
        for hd in (2, 48, 64, 128):
            for heads in (1, 6):
                for Lq in (1, 16):
                    for B in (1, 3):
                        _rope_case(hp, L, rng, B, Lq, heads, hd)


def check_rope_past_the_stream_grid_cap(dev):
    """stream_grid caps at 2048 workgroups of 256 threads, and the RoPE launches ask for one thread per two pairs: 683 x 8
    rows of 6 x 32 pairs (12 x 32 for the packed form) are 1,049,088 pairs, a little over 2^20, so every thread takes a
    third pair."""
    hp, L, device = _env(dev)
    with device:
        _rope_case(hp, L, np.random.default_rng(242), 683, 8, 6, 64)


# =====================================================================================================================
# SiLU / SwiGLU, the device-scalar scale
# =====================================================================================================================
SPECIAL_G = (-100.0, -20.0, 0.0, 20.0, 100.0)


def _swiglu_case(hp, L, rng, n, off, with_u, g=None):
    what = ("swiglu", n, off, with_u)
    g = rng.standard_normal(n).astype(F32) * 3 if g is None else np.asarray(g, F32)
    u = rng.standard_normal(n).astype(F32) if with_u else None
    dy = rng.standard_normal(n).astype(F32)
    G, DY, Y, DG = Buf(hp, g, off), Buf(hp, dy, off), Buf(hp, _nan(n), off), Buf(hp, _nan(n), off)
    U, DU = (Buf(hp, u, off), Buf(hp, _nan(n), off)) if with_u else (None, None)
    with np.errstate(all="ignore"):
        L.call("pdn_swiglu_fwd_f32", G.ptr, U.ptr if U else None, Y.ptr, n, hp.stream())
        L.call("pdn_swiglu_bwd_f32", G.ptr, U.ptr if U else None, DY.ptr, DG.ptr, DU.ptr if DU else None, n, hp.stream())
    dg_ref, du_ref = ref.swiglu_bwd(g, u, dy)
    y, dg = Y.get(), DG.get()
    assert np.isfinite(y).all() and np.isfinite(dg).all(), what
    _close(y, ref.swiglu_fwd(g, u), what + ("y",))
    _close(dg, dg_ref, what + ("dg",))
    if with_u:
        _close(DU.get(), du_ref, what + ("du",))


def check_swiglu_vector_and_scalar_paths(dev):
    """swiglu_fwd_kernel / swiglu_bwd_kernel: the float4 body with its scalar tail (n = 1, 3: tail only; 4: body only;
    1027: both), the scalar path behind bases 4 bytes off the 16-byte grid, u = NULL (plain SiLU), and gates of -100, -20,
    0, 20, 100, where exp(-g) overflows or vanishes: outputs finite."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(251)
    with device:
        for n in (1, 3, 4, 1027):
            for off in (0, 1):
                for with_u in (True, False):
                    _swiglu_case(hp, L, rng, n, off, with_u)
        for off in (0, 1):
            for with_u in (True, False):
                _swiglu_case(hp, L, rng, 8, off, with_u, g=SPECIAL_G + (1.0, -1.0, 5.0))


def check_swiglu_rows_packed(dev):
    """swiglu_rows_fwd_kernel / swiglu_rows_bwd_kernel on a packed gate | up projection (rows, 2F): F of one and two
    float4 and 772 (193 float4: no multiple of the workgroup), 1, 3 and 1000 rows, against the unpacked statement;
    F % 4 != 0 and misaligned operands are refused on the host."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(252)
    with device:
        for F in (4, 8, 772):
            for rows in (1, 3, 1000):
                what = ("swiglu_rows", rows, F)
                gu = rng.standard_normal((rows, 2 * F)).astype(F32) * 3
                gu[0, :4] = (-100.0, 100.0, 0.0, -20.0)
                dy = rng.standard_normal((rows, F)).astype(F32)
                GU, DY, Y, DGU = Buf(hp, gu), Buf(hp, dy), Buf(hp, _nan((rows, F))), Buf(hp, _nan((rows, 2 * F)))
                with np.errstate(all="ignore"):
                    L.call("pdn_swiglu_rows_fwd_f32", GU.ptr, Y.ptr, rows, F, hp.stream())
                    L.call("pdn_swiglu_rows_bwd_f32", GU.ptr, DY.ptr, DGU.ptr, rows, F, hp.stream())
                dg_ref, du_ref = ref.swiglu_bwd(gu[:, :F], gu[:, F:], dy)
                _close(Y.get(), ref.swiglu_fwd(gu[:, :F], gu[:, F:]), what + ("y",))
                _close(DGU.get()[:, :F], dg_ref, what + ("dgate",))
                _close(DGU.get()[:, F:], du_ref, what + ("dup",))
        GU, DY, Y, DGU = Buf(hp, np.ones(64, F32)), Buf(hp, np.ones(32, F32)), Buf(hp, _nan(32)), Buf(hp, _nan(64))
        st = hp.stream()
        _refused(L, EINVAL, "pdn_swiglu_rows_fwd_f32", GU.ptr, Y.ptr, 2, 6, st)
        _refused(L, EINVAL, "pdn_swiglu_rows_bwd_f32", GU.ptr, DY.ptr, DGU.ptr, 2, 6, st)
        _refused(L, EINVAL, "pdn_swiglu_rows_fwd_f32", GU.ptr + 4, Y.ptr, 2, 8, st)
        _refused(L, EINVAL, "pdn_swiglu_rows_fwd_f32", GU.ptr, Y.ptr + 4, 2, 8, st)
        _refused(L, EINVAL, "pdn_swiglu_rows_bwd_f32", GU.ptr, DY.ptr + 4, DGU.ptr, 2, 8, st)
        _refused(L, EINVAL, "pdn_swiglu_rows_bwd_f32", GU.ptr, DY.ptr, DGU.ptr + 4, 2, 8, st)
        assert np.isnan(Y.get()).all() and np.isnan(DGU.get()).all(), "written by a refused call"


def check_scale_by_device_scalar(dev):
    """scale_by_device_scalar_kernel: a scalar of exactly 1 leaves the buffer bit-identical (the blocks return after one
    load); 0 and -2.5 are one float32 product per element; n = 1, 5, 1027."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(253)
    with device:
        for n in (1, 5, 1027):
            x = rng.standard_normal(n).astype(F32)
            for s in (1.0, 0.0, -2.5):
                X, S = Buf(hp, x), Buf(hp, np.array([s], F32))
                L.call("pdn_scale_by_device_scalar_f32", X.ptr, n, S.ptr, hp.stream())
                got = X.get()
                assert np.array_equal(got, x * F32(s)), (n, s)
                if s == 1.0:
                    assert got.tobytes() == x.tobytes(), (n, "scalar 1 changed the buffer")


# =====================================================================================================================
# Adam
# =====================================================================================================================
ADAM = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, gs=0.5)


def _adam_chunks(hp, rng):
    """(size, offset in floats) per chunk: sizes 1, 3, 5 (tail only / body + tail), 16384, one chunk 4 bytes off the 16-byte
    grid (scalar path), one with an all-zero gradient, one with zero gradient AND zero weights (0 / (0 + eps))."""
    host, dev = [], []
    for n, off, kind in ((1, 0, ""), (3, 0, ""), (5, 0, ""), (16384, 0, ""), (37, 1, ""), (9, 0, "g0"), (6, 0, "p0g0")):
        p = rng.standard_normal(n).astype(F32)
        g = rng.standard_normal(n).astype(F32)
        m, v = 0.1 * rng.standard_normal(n).astype(F32), (0.01 * rng.random(n)).astype(F32)
        if kind:
            g[:] = 0
        if kind == "p0g0":
            p[:], m[:], v[:] = 0, 0, 0
        host.append([p, g, m, v])
        dev.append([Buf(hp, a, off) for a in (p, g, m, v)])
    table = np.array([[b.ptr for b in bufs] + [len(h[0])] for bufs, h in zip(dev, host)], np.int64)
    return host, dev, Buf(hp, table, dtype=np.int64)


def _adam_check(host, dev, what):
    for k, (h, d) in enumerate(zip(host, dev)):
        for name, a, b in zip("pgmv", h, d):
            got = b.get()
            assert np.isfinite(got).all(), what + (k, name)
            _close(got, a, what + ("chunk", k, name))
    assert not host[-1][0].any() and not dev[-1][0].get().any(), what + ("0 / (0 + eps) moved a zero weight",)


def check_adam_multi(dev):
    """adam_multi_kernel over three steps with weight_decay != 0 and grad_scale != 1, one workgroup per chunk: the float4
    body, its tail, the scalar path of a chunk off the 16-byte grid, an all-zero gradient -- against float64 after every
    step."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(261)
    A = ADAM
    with device:
        host, dev_, TABLE = _adam_chunks(hp, rng)
        host = [[a.astype(F64) for a in h] for h in host]
        for t in (1, 2, 3):
            step = ref.adam_step_size(A["lr"], A["b1"], A["b2"], t)
            L.call("pdn_adam_multi_f32", TABLE.ptr, len(host), step, A["b1"], A["b2"], 1 - A["b1"], 1 - A["b2"], A["eps"],
                   A["wd"], A["gs"], hp.stream())
            for h in host:
                h[0], h[2], h[3] = ref.adam_step(h[0], h[1], h[2], h[3], step, A["b1"], A["b2"], A["eps"], A["wd"], A["gs"])
            _adam_check(host, dev_, ("adam", t))


def check_adam_multi_tick(dev):
    """adam_tick_kernel + adam_multi_kernel reading its step size from the device (the replayed optimizer step): the
    device counter advances by one per call and step_dev = lr * sqrt(1 - b2^t) / (1 - b1^t) for t = 1..3; the update
    follows the float64 statement with that step.  (The emulator has no such entry: real library only.)"""
    hp, L, device = _env(dev)
    if _emulated(L):
        return
    rng = np.random.default_rng(262)
    A = ADAM
    b1, b2 = float(F32(A["b1"])), float(F32(A["b2"]))                          # the entry takes floats
    with device:
        host, dev_, TABLE = _adam_chunks(hp, rng)
        host = [[a.astype(F64) for a in h] for h in host]
        STATE, STEP = Buf(hp, np.array([1.0, A["lr"]]), dtype=F64), Buf(hp, _nan(1))
        for t in (1, 2, 3):
            L.call("pdn_adam_multi_tick_f32", TABLE.ptr, len(host), STATE.ptr, STEP.ptr, A["b1"], A["b2"], A["eps"], A["wd"],
                   A["gs"], hp.stream())
            want = ref.adam_step_size(A["lr"], b1, b2, t)
            got = float(STEP.get()[0])
            assert abs(got - want) <= 2.0 ** -23 * want, ("step_dev", t, got, want)        # one float32 rounding
            assert np.array_equal(STATE.get(), [t + 1.0, A["lr"]]), ("device step counter", t, STATE.get())
            for h in host:
                h[0], h[2], h[3] = ref.adam_step(h[0], h[1], h[2], h[3], got, b1, b2, A["eps"], A["wd"], A["gs"])
            _adam_check(host, dev_, ("adam tick", t))


# =====================================================================================================================
# reductions
# =====================================================================================================================
ROP = {"sum": 0, "mean": 1, "max": 2, "min": 3, "argmax": 4, "argmin": 5}


def _reduce(hp, L, X, ptr, shape, strides, axes, op, ws_bytes=None):
    """pdn_reduce of the float32 view (ptr, shape, element strides) of device array X over `axes`."""
    nd = len(shape)
    kept = tuple(s for i, s in enumerate(shape) if i not in axes)
    outn = max(int(np.prod(kept)), 1)
    OUT = Buf(hp, np.zeros(outn, np.int64 if op.startswith("arg") else F32), dtype=np.int64 if op.startswith("arg") else F32)
    ws_ptr, ws_have = hp.workspace(outn * 1024 * 16 + 4096 if outn <= 4096 else outn * 16 * 64)
    flags = (ctypes.c_uint8 * nd)(*[1 if i in axes else 0 for i in range(nd)])
    L.call("pdn_reduce", 0, ROP[op], nd, (ctypes.c_int64 * nd)(*shape), (ctypes.c_int64 * nd)(*strides), flags, ptr, OUT.ptr,
           ws_ptr, ws_have if ws_bytes is None else ws_bytes, hp.stream())
    return OUT.get().reshape(kept)


def check_reduce_colsum4_and_its_neighbours(dev):
    """reduce_colsum4_kernel (float32 sum / mean over axis 0 with outN >= 256, outN % 4 == 0, R >= 4096, ld % 4 == 0,
    16-byte bases): the smallest shape, one with a last workgroup of one thread column and a row tail, 8195 x 1024 (the
    unrolled loop, its tail and several chunks), and a column slice (ld != outN).  Its neighbours take reduce_col_kernel:
    outN = 258, R = 4095, a slice starting at column 1 (base off the 16-byte grid).  With a workspace too small for the
    partials the reduction runs as one chunk."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(271)
    with device:
        for R, N, lo, hi in ((4096, 256, 0, 256), (4100, 260, 0, 260), (8195, 1024, 0, 1024), (4100, 260, 0, 256),
                             (4100, 258, 0, 258), (4095, 256, 0, 256), (4100, 260, 1, 257)):
            x = (rng.standard_normal((R, N)) + 0.5).astype(F32)
            X = hp.from_numpy(x)
            want = x[:, lo:hi].astype(F64).sum(0)
            for op, w in (("sum", want), ("mean", want / R)):
                _sumtol(_reduce(hp, L, X, X._ptr + 4 * lo, (R, hi - lo), (N, 1), (0,), op), w, (R, N, lo, hi, op))
                _sumtol(_reduce(hp, L, X, X._ptr + 4 * lo, (R, hi - lo), (N, 1), (0,), op, ws_bytes=4 * (hi - lo)), w,
                        (R, N, lo, hi, op, "small workspace"))


def _with_specials(rng, shape, axis, spots):
    """Standard normal data with `spots` = ((position along the reduced axis, value), ...) planted in EVERY reduced run."""
    x = (rng.standard_normal(shape) + 0.5).astype(F32)                   # (+ 0.5: a finite sum stays away from 0)
    for pos, val in spots:
        x[(slice(None),) * axis + (pos,)] = val
    return x


def check_reduce_nan_and_infinity(dev):
    """reduce_row_kernel (3 x 70000 over the last axis, 70000 flat: several chunks of 256 threads) and reduce_col_kernel
    (5000 x 33 over axis 0: 4 row lanes x 78 chunks) with a NaN, +inf or -inf first, last or mid-run, two NaNs, and a NaN
    after an infinity: max / min / sum / argmax / argmin answer as NumPy does (a NaN beats every number and the first
    one's index wins, wherever it falls in the thread, shuffle and chunk order)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(272)
    nan, inf = np.nan, np.inf
    with device, np.errstate(all="ignore"):
        for shape, axis in (((3, 70000), 1), ((70000,), 0), ((5000, 33), 0)):
            R = shape[axis]
            strides = (shape[1], 1) if len(shape) == 2 else (1,)
            mid, late = R // 2 + 37, R - 1000
            plans = [((p, v),) for v in (nan, inf, -inf) for p in (0, R - 1, mid)]
            plans += [((mid, nan), (late, nan)), ((0, inf), (mid, nan), (late, nan)), ((3, -inf), (late, nan)),
                      ((mid, inf), (late, inf)), ((mid, -inf), (late, -inf))]
            for spots in plans:
                x = _with_specials(rng, shape, axis, spots)
                X = hp.from_numpy(x)
                for op in ("max", "min", "argmax", "argmin", "sum"):
                    got = _reduce(hp, L, X, X._ptr, shape, strides, (axis,), op)
                    want = getattr(np, op)(x.astype(F64), axis=axis)
                    what = (shape, spots, op)
                    if op.startswith("arg"):
                        assert np.array_equal(got, want), what + (got, want)
                    else:
                        fin = np.isfinite(want)
                        assert np.array_equal(np.asarray(got)[~fin], np.asarray(want)[~fin], equal_nan=True), what + (got, want)
                        if fin.any():
                            _sumtol(np.asarray(got)[fin], np.asarray(want)[fin], what)


def check_reduce_arg_ties(dev):
    """argmax / argmin over runs of equal values: the first index wins, through every thread, wave, lane and chunk merge
    (the same three shapes); and a run whose extreme value appears twice."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(273)
    with device:
        for shape, axis in (((3, 70000), 1), ((70000,), 0), ((5000, 33), 0)):
            strides = (shape[1], 1) if len(shape) == 2 else (1,)
            R = shape[axis]
            flat_ = np.full(shape, 2.5, F32)
            twice = _with_specials(rng, shape, axis, ((R // 2 + 37, 9.0), (R - 1000, 9.0)))
            twice_low = _with_specials(rng, shape, axis, ((R // 3 + 5, -9.0), (R - 7, -9.0)))
            for x in (flat_, twice, twice_low):
                X = hp.from_numpy(x)
                for op in ("argmax", "argmin"):
                    got = _reduce(hp, L, X, X._ptr, shape, strides, (axis,), op)
                    assert np.array_equal(got, getattr(np, op)(x, axis=axis)), (shape, op, got)


for _fn in [v for k, v in sorted(globals().items()) if k.startswith("check_")]:
    device_variants(globals(), _fn)
