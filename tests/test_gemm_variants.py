"""pdn_gemm_f32 (csrc/gemm.hip) at every kernel its host code can choose, each pinned with the routing variables and PROVED by
the line PDN_GEMM_DEBUG prints: the thirteen tile configurations in the four operand layouts, scalar staging, the fused
column sums, the bit-mask epilogues of pdn_linear_relu_fwd_f32 / pdn_linear_dx_masked_f32, the k-split with both forms of
the slab reduce, batches, degenerate extents, the grid's y limit, and the wave-streaming weight-gradient kernels of
csrc/gemm_stream.h.  A case whose route is not the one it was written for fails.

Every check is one `_run_case`; each GPU test (`-m gpu`) has a twin that runs the same case list on the NumPy emulation of
the C ABI, which has no dispatch: the twin checks the harness, the float64 statements (tests/gemm_variants_ref.py) and the
operand plumbing (the selection itself, csrc/gemm_select.h, is held to the same pinned routes without a GPU by
tests/test_gemm_select_cpu.py).  The `test_harness_notices_*` tests show that `_run_case` fails on an entry with one defect.

Criteria, per case:
  * exact pass: operands, bias, residual and prior C are integers in [-4, 4], alpha in {1, 0.5, 2}, beta in {0, 1, 2},
    K <= 4224: every partial sum is a multiple of 1/2 below 2^18, exact in fp32 in any order -- `np.array_equal` against
    float64.  Catches a dropped contraction index, a shifted bias, a swapped tile, a wrong slab.
  * precision pass: the same case on standard-normal data, max-norm relative error against float64 below 2e-5 (the
    criterion of test_gemm_mid_size_dispatch_edges); the error is printed per case (an MI355X run:
    profiles/gemm_variants_gpu_tests.txt).  Integers are exact in bf16 / xf32 too: this pass notices a reduced-precision
    matrix instruction.
  * guards: every buffer has guard elements on both sides (Buf of tests/test_row_kernels.py); the padding columns of an
    ldc > N output and two rows beyond M are prefilled with NaN and must come back bit-identical; with beta = 0 the
    output itself is prefilled with NaN (it must not be read); the inputs come back unchanged.
  * determinism: a case with more than one split runs twice, bit-equal.

Layouts: A is row-major (akin=1) or a .T view (`at`: m-contiguous, akin=0); B is row-major (bkin=0) or a .T view (`bt`:
k-contiguous, bkin=1).  NN / NT / TN / TT name (at, bt) = (0,0) / (0,1) / (1,0) / (1,1); TN is the x^T g form."""
import os
import re
import sys
import zlib
from dataclasses import dataclass, field

import numpy as np
import pytest

from tests import gemm_variants_ref as ref
from tests.test_row_kernels import Buf, _emulated, _refused

F32, F64, U32 = np.float32, np.float64, np.uint32
TOL = 2e-5                                   # test_gemm_mid_size_dispatch_edges (tests/test_kernels_gpu.py)
EINVAL, EUNSUPPORTED = -1, -2
# every variable pdn_gemm_f32 reads per call; none may leak from one case into the next (PDN_GEMM_NO_FIXED is cached in a
# static on first use and is left alone)
ROUTING_VARS = ("PDN_GEMM_CFG", "PDN_GEMM_STREAM_SHAPE", "PDN_GEMM_STREAM_SPLITS", "PDN_GEMM_STREAM_DIRECT",
                "PDN_GEMM_STREAM_NODMA", "PDN_GEMM_STREAM_MAX", "PDN_GEMM_NO_STREAM", "PDN_GEMM_NO_NARROW", "PDN_GEMM_DEBUG")

# kCfgs of csrc/gemm_select.h: (waves_m, waves_n, wm, wn, BK); BM = 32 waves_m wm, BN = 32 waves_n wn
KCFGS = ((2, 2, 2, 2, 32), (4, 1, 1, 3, 32), (1, 4, 3, 1, 32), (4, 1, 1, 2, 32), (1, 4, 2, 1, 32), (2, 2, 1, 1, 32),
         (2, 2, 4, 2, 16), (2, 2, 2, 4, 16), (4, 1, 2, 3, 16), (1, 4, 3, 2, 16), (2, 1, 1, 3, 32), (1, 2, 3, 1, 32),
         (4, 1, 1, 3, 16))
MASK_CFGS = (0, 3, 5, 6, 7, 8)               # the tile shapes built with MASKS
STREAM_SHAPES = ((3, 3), (5, 2), (2, 5), (4, 2), (2, 4))      # kShapes of csrc/gemm_select.h, in 32-row / 32-column tiles
LAYOUTS = (("NN", False, False), ("NT", False, True), ("TN", True, False), ("TT", True, True))


def tile(c):
    wmv, wnv, wm, wn, bk = KCFGS[c]
    return 32 * wmv * wm, 32 * wnv * wn, bk


@dataclass
class Case:
    name: str
    M: int
    N: int
    K: int
    at: bool = False                         # A is a .T view
    bt: bool = False                         # B is a .T view
    alpha: float = 1.0
    beta: float = 0.0
    bias: bool = False
    res: bool = False
    ldc_pad: int = 0                         # ldc = N + ldc_pad
    a_off: int = 0                           # elements (4 bytes each) that a base is off the 16-byte grid
    b_off: int = 0
    bias_off: int = 0
    ws_off: int = 0
    a_pad: int = 0                           # extra elements in an operand's row stride
    b_pad: int = 0
    nb: tuple = (1, 1)
    gaps: tuple = ((0, 0), (0, 0), (0, 0))   # extra elements in the (outer, inner) batch strides of A, B, C
    a_bcast: bool = False                    # A shared by the batch: batch strides 0
    slabs: int = 0                           # workspace for this many slabs of the whole output (0: none passed)
    colsum: int = -1                         # b_colsum: -1 none, 0 overwrite, 1 accumulate
    env: dict = field(default_factory=dict)
    route: dict = field(default_factory=dict)   # what the debug line must say: family, cfg, akin, bkin, vec, splits, sshape, kind
    entry: str = "gemm"                      # "gemm" | "relu" (pdn_linear_relu_fwd_f32) | "dx" (pdn_linear_dx_masked_f32)
    existing: bool = False                   # dx: an `existing` gradient is added
    partials: bool = False                   # dx: the 32-row partial column sums are asked for
    refuse: int = 0                          # the status a refused call returns (0: the call succeeds)
    writes: bool = True                      # False: an empty extent, nothing may be written


# =====================================================================================================================
# the harness
# =====================================================================================================================
def _layout(rows, cols, trans, pad, nb, gap=(0, 0), bcast=False, extra_rows=0):
    """Element strides and allocation size of a batched (rows x cols) operand: row-major with row stride cols + pad, or
    (trans) stored as its transpose with row stride rows + pad."""
    ld = (rows if trans else cols) + pad
    rs, cs = (1, ld) if trans else (ld, 1)
    per = ((cols if trans else rows) + extra_rows) * ld
    bs2 = per + gap[1]
    bs1 = nb[1] * bs2 + gap[0]
    if bcast:
        bs1 = bs2 = 0
    size = max(nb[0] - 1, 0) * bs1 + max(nb[1] - 1, 0) * bs2 + per
    return (nb[0], nb[1], rows, cols), (bs1, bs2, rs, cs), size


def _logical(host, shape, strides):
    if 0 in shape:
        return np.zeros(shape, host.dtype)
    return np.lib.stride_tricks.as_strided(host, shape, [s * host.itemsize for s in strides])


def _gen(rng, kind):
    if kind == "exact":
        return lambda n: rng.integers(-4, 5, int(n)).astype(F32)
    return lambda n: rng.standard_normal(int(n)).astype(F32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(U32), np.ascontiguousarray(b).view(U32))


_LINE = re.compile(r"pdn_gemm_f32 M=(\d+) N=(\d+) K=(\d+) nb=(\d+) akin=(\d) bkin=(\d) vec=(\d) -> (\w+) cfg=(\d+) "
                   r"splits=(\d+)(?: sshape=(\d+) kind=([\w-]+))?")


def _drain(capfd):
    """What the library wrote to stderr since the last call; the test's own prints are handed on to pytest's report."""
    out, err = capfd.readouterr()
    sys.stdout.write(out)
    return err


def _check_route(case, err):
    """The one line PDN_GEMM_DEBUG printed for this call says what the case was written for."""
    found = [m for m in map(_LINE.search, err.splitlines()) if m]
    assert len(found) == 1, (case.name, "expected one route line", err)
    g = found[0].groups()
    got = dict(M=int(g[0]), N=int(g[1]), K=int(g[2]), nb=int(g[3]), akin=int(g[4]), bkin=int(g[5]), vec=int(g[6]),
               family=g[7], cfg=int(g[8]), splits=int(g[9]), sshape=None if g[10] is None else int(g[10]), kind=g[11])
    want = dict(M=case.M, N=case.N, K=case.K, nb=case.nb[0] * case.nb[1], **case.route)
    for key in ("family", "cfg", "akin", "bkin", "vec"):
        assert key in want, (case.name, "the case does not pin", key)
    if want["family"] == "stream":
        assert "sshape" in want and "kind" in want and "splits" in want, (case.name, "a stream case pins shape, kind, splits")
    wrong = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not wrong, (case.name, "routed elsewhere: (got, wanted)", wrong, found[0].group(0))
    return got


def _set_env(case, monkeypatch, debug):
    for v in ROUTING_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in case.env.items():
        assert k in ROUTING_VARS, k
        monkeypatch.setenv(k, v)
    if debug:
        monkeypatch.setenv("PDN_GEMM_DEBUG", "1")


def _clear_env(monkeypatch):
    for v in ROUTING_VARS:
        monkeypatch.delenv(v, raising=False)
    assert not any(v in os.environ for v in ROUTING_VARS)


def _workspace(hp, case, floats):
    if not case.slabs:
        return None, 0
    nbytes = int(floats) * 4 * case.slabs
    ptr, have = hp.workspace(nbytes + 16)
    assert have >= nbytes + 16
    return ptr + 4 * case.ws_off, nbytes


def _judge(case, kind, what, got, want):
    """Exact pass: equality with float64; precision pass: the printed max-norm relative error below TOL."""
    assert got.shape == want.shape, (case.name, what, got.shape, want.shape)
    if kind == "exact":
        if not np.array_equal(got.astype(F64), want):
            bad = np.argwhere(got.astype(F64) != want)
            i = tuple(bad[0])
            raise AssertionError((case.name, what, "not exact", len(bad), "elements, first at", i, float(got[i]), float(want[i])))
        return
    assert np.isfinite(got).all(), (case.name, what, "not finite")
    err = ref.rel_err(got, want)
    print(f"{case.name} | {what}: rel err {err:.3e}")
    assert err < TOL, (case.name, what, err)


def _gemm_pass(hp, L, case, kind, capfd):
    c = case
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) + (kind == "exact"))
    gen = _gen(rng, kind)
    a_shape, a_str, a_n = _layout(c.M, c.K, c.at, c.a_pad, c.nb, c.gaps[0], c.a_bcast)
    b_shape, b_str, b_n = _layout(c.K, c.N, c.bt, c.b_pad, c.nb, c.gaps[1])
    c_shape, c_str, c_n = _layout(c.M, c.N, False, c.ldc_pad, c.nb, c.gaps[2], extra_rows=2)
    a_host, b_host = gen(a_n), gen(b_n)
    bias_host = gen(c.N) if c.bias else None
    res_host = gen(c_n) if c.res else None
    cs_host = gen(c.N) if c.colsum >= 0 else None
    c_host = np.full(c_n, np.nan, F32)
    if c.beta != 0.0:
        _logical(c_host, c_shape, c_str)[...] = gen(int(np.prod(c_shape))).reshape(c_shape)
    inside = np.zeros(c_n, bool)
    if c.writes and not c.refuse:
        _logical(inside, c_shape, c_str)[...] = True
    a64, b64 = _logical(a_host, a_shape, a_str).astype(F64), _logical(b_host, b_shape, b_str).astype(F64)
    want = ref.gemm(a64, b64, c.alpha, bias_host, None if res_host is None else _logical(res_host, c_shape, c_str),
                    c.beta, _logical(c_host, c_shape, c_str))
    A, B = Buf(hp, a_host, c.a_off), Buf(hp, b_host, c.b_off)
    BIAS = Buf(hp, bias_host, c.bias_off) if c.bias else None
    RES = Buf(hp, res_host) if c.res else None
    ws_ptr, ws_bytes = _workspace(hp, c, int(np.prod(c_shape)))
    ldc = c.N + c.ldc_pad

    def once():
        C = Buf(hp, c_host)
        CS = Buf(hp, cs_host) if c.colsum >= 0 else None
        args = (c.M, c.N, c.K, c.alpha, A.ptr, a_str[2], a_str[3], B.ptr, b_str[2], b_str[3], c.beta, C.ptr, ldc,
                BIAS.ptr if BIAS else None, c.nb[0], c.nb[1], a_str[0], a_str[1], b_str[0], b_str[1], c_str[0], c_str[1],
                RES.ptr if RES else None, CS.ptr if CS else None, max(c.colsum, 0), ws_ptr, ws_bytes, hp.stream())
        _drain(capfd)
        if c.refuse:
            _refused(L, c.refuse, "pdn_gemm_f32", *args)
        else:
            L.call("pdn_gemm_f32", *args)
        return C.get(), (CS.get() if CS else None), _drain(capfd)

    h, cs, err = once()
    got_route = None
    if not _emulated(L):
        if c.writes and not c.refuse:
            got_route = _check_route(c, err)
        elif not c.writes:                   # (a refusal may come after the line: the library prints before its last check)
            assert not _LINE.search(err), (c.name, "an empty product printed a route", err)
    assert _same_bits(h[~inside], c_host[~inside]), (c.name, "padding columns, rows beyond M or an untouched output changed")
    if c.writes and not c.refuse:
        _judge(c, kind, "C", _logical(h, c_shape, c_str), want)
        if c.colsum >= 0:
            _judge(c, kind, "colsum", cs, ref.colsum(b64[0, 0], cs_host, c.colsum))
        if (got_route["splits"] if got_route else c.route.get("splits", 1)) > 1:
            h2, cs2, _ = once()
            assert _same_bits(h2, h) and (cs is None or _same_bits(cs2, cs)), (c.name, "two runs differ")
    elif c.colsum >= 0:
        assert _same_bits(cs, cs_host), (c.name, "a refused call wrote the column sums")
    assert _same_bits(A.get(), a_host) and _same_bits(B.get(), b_host), (c.name, "an operand changed")
    assert BIAS is None or _same_bits(BIAS.get(), bias_host), (c.name, "the bias changed")
    assert RES is None or _same_bits(RES.get(), res_host), (c.name, "the residual changed")


def _mask_pass(hp, L, case, kind, capfd):
    """pdn_linear_relu_fwd_f32 (h = max(0, x W + bias) and the bits z >= 0) or pdn_linear_dx_masked_f32 (dx = bits o (g W^T
    + existing) and its 32-row partial column sums), stated as the product A (M x K) B (K x N): for the forward B is W,
    for the masked gradient B is W^T (so `bt` is a row-major W)."""
    c = case
    assert not c.at and c.nb == (1, 1) and c.N % 32 == 0
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) + (kind == "exact"))
    gen = _gen(rng, kind)
    a_shape, a_str, a_n = _layout(c.M, c.K, False, c.a_pad, (1, 1))
    b_shape, b_str, b_n = _layout(c.K, c.N, c.bt, c.b_pad, (1, 1))
    c_shape, c_str, c_n = _layout(c.M, c.N, False, c.ldc_pad, (1, 1), extra_rows=2)
    a_host, b_host = gen(a_n), gen(b_n)
    a64, b64 = _logical(a_host, a_shape, a_str)[0, 0].astype(F64), _logical(b_host, b_shape, b_str)[0, 0].astype(F64)
    A, B = Buf(hp, a_host, c.a_off), Buf(hp, b_host, c.b_off)
    c_host = np.full(c_n, np.nan, F32)
    inside = np.zeros(c_n, bool)
    _logical(inside, c_shape, c_str)[...] = True
    C = Buf(hp, c_host)
    ld = c.N + c.ldc_pad
    words = c.N // 32
    _drain(capfd)
    if c.entry == "relu":
        bias_host = gen(c.N) if c.bias else None
        BIAS = Buf(hp, bias_host, c.bias_off) if c.bias else None
        MASK = Buf(hp, np.full((c.M, words), 0x5A5A5A5A, np.int32), dtype=np.int32)
        L.call("pdn_linear_relu_fwd_f32", A.ptr, a_str[2], B.ptr, b_str[2], b_str[3], BIAS.ptr if BIAS else None, C.ptr, ld,
               MASK.ptr, c.M, c.N, c.K, hp.stream())
        err = _drain(capfd)
        z, h_want, keep = ref.linear_relu(a64, b64, bias_host)
        h = C.get()
        _judge(c, kind, "h", _logical(h, c_shape, c_str)[0, 0], h_want)
        bits = ref.unpack_bits(MASK.get().view(U32), c.N)
        # exact pass: the bits ARE z >= 0, zeros included; precision pass: wherever z is further from 0 than its error bound
        sure = np.ones_like(keep) if kind == "exact" else np.abs(z) > TOL * np.abs(z).max()
        assert np.array_equal(bits[sure], keep[sure]), (c.name, "relu bits", int((bits != keep)[sure].sum()))
        assert BIAS is None or _same_bits(BIAS.get(), bias_host), (c.name, "the bias changed")
    else:
        keep = rng.random((c.M, c.N)) < 0.6
        mask_host = ref.pack_bits(keep).view(np.int32)
        MASK = Buf(hp, mask_host, dtype=np.int32)
        ex_host = gen(c_n) if c.existing else None
        EX = Buf(hp, ex_host) if c.existing else None
        nband = (c.M + 31) // 32
        PART = Buf(hp, np.full((nband, c.N), np.nan, F32)) if c.partials else None
        # W (fin x fout) = B^T: its strides are B's, swapped
        L.call("pdn_linear_dx_masked_f32", A.ptr, a_str[2], B.ptr, b_str[3], b_str[2], C.ptr, ld, EX.ptr if EX else None,
               MASK.ptr, PART.ptr if PART else None, c.M, c.N, c.K, hp.stream())
        err = _drain(capfd)
        dx_want, part_want = ref.dx_masked(a64, b64.T, keep, None if ex_host is None else _logical(ex_host, c_shape, c_str)[0, 0])
        h = C.get()
        dx = _logical(h, c_shape, c_str)[0, 0]
        assert np.all(dx[~keep] == 0.0), (c.name, "masked-out entries are not exactly 0")
        _judge(c, kind, "dx", dx, dx_want)
        if c.partials:
            _judge(c, kind, "partials", PART.get(), part_want)
        assert np.array_equal(MASK.get(), mask_host), (c.name, "the gradient bits changed")
        assert EX is None or _same_bits(EX.get(), ex_host), (c.name, "`existing` changed")
    if not _emulated(L):
        _check_route(c, err)
    assert _same_bits(h[~inside], c_host[~inside]), (c.name, "padding columns or rows beyond M changed")
    assert _same_bits(A.get(), a_host) and _same_bits(B.get(), b_host), (c.name, "an operand changed")


def _run_case(hp, L, case, monkeypatch, capfd, passes=("exact", "precision")):
    """One case through both passes, with its routing variables set for the call and gone afterwards."""
    assert case.K <= 4224 and case.alpha in (1.0, 0.5, 2.0) and case.beta in (0.0, 1.0, 2.0), case.name
    _set_env(case, monkeypatch, debug=not _emulated(L))
    try:
        for kind in passes:
            (_gemm_pass if case.entry == "gemm" else _mask_pass)(hp, L, case, kind, capfd)
    finally:
        _clear_env(monkeypatch)


def _register(name, make_cases, values=None):
    """`test_<name>_gpu` (marked gpu) and its twin `test_<name>_emulated` over make_cases([value])."""
    def run(hp, monkeypatch, capfd, *v):
        from pydynet_amd import _lib
        L = _lib.lib()
        cases = make_cases(*v)
        assert cases and len({c.name for c in cases}) == len(cases)
        for case in cases:
            _run_case(hp, L, case, monkeypatch, capfd)

    if values is None:
        @pytest.mark.gpu
        def on_gpu(hip, monkeypatch, capfd):
            run(hip, monkeypatch, capfd)

        def on_emulator(emulated_hip, monkeypatch, capfd):
            run(emulated_hip, monkeypatch, capfd)
    else:
        @pytest.mark.gpu
        @pytest.mark.parametrize("v", values)
        def on_gpu(hip, monkeypatch, capfd, v):
            run(hip, monkeypatch, capfd, v)

        @pytest.mark.parametrize("v", values)
        def on_emulator(emulated_hip, monkeypatch, capfd, v):
            run(emulated_hip, monkeypatch, capfd, v)
    on_gpu.__doc__ = on_emulator.__doc__ = make_cases.__doc__
    globals()[f"test_{name}_gpu"] = on_gpu
    globals()[f"test_{name}_emulated"] = on_emulator


# =====================================================================================================================
# tiled kernel: every configuration x layout
# =====================================================================================================================
EPILOGUES = (("plain", dict()),
             ("a.5+bias+b2", dict(alpha=0.5, bias=True, beta=2.0)),
             ("res,ldc=N+4", dict(res=True, ldc_pad=4)),
             ("bias,ldc=N+1", dict(bias=True, ldc_pad=1)),                # the scalar epilogue on full tiles
             ("bias 4B off", dict(bias=True, bias_off=1)))
FULL = dict(alpha=0.5, bias=True, res=True, beta=2.0)


def _tiled(c, at, bt, splits=1, **more):
    return dict(at=at, bt=bt, slabs=splits if splits > 1 else 0, env={"PDN_GEMM_CFG": f"{c},{splits}"},
                route=dict(family="tiled", cfg=c, akin=int(not at), bkin=int(bt), vec=1, splits=splits), **more)


def tiled_cases(c):
    """gemm_f32_mfma_kernel<kCfgs[c], A_KIN, B_KIN, VEC> in the four layouts.  M = 8 BM + 40: nine row tiles (a ragged last
    super-tile group of one, a tile count that is no multiple of 8 for the XCD remap) whose last has 40 rows; N = 2 BN + 36:
    a 36-column edge tile.  K = 96 unsplit (whole k-tiles: the interior loop, with the clamped init_offsets of
    configurations 8, 9, 12) and K = 5 BK + 12 over 3 splits (2 BK, 2 BK, BK + 12: full tiles through the bounds-tested
    loop).  The five epilogues are dealt round-robin (test_case_tables_cover_what_they_claim)."""
    BM, BN, BK = tile(c)
    M, N = 8 * BM + 40, 2 * BN + 36
    out = []
    for li, (ln, at, bt) in enumerate(LAYOUTS):
        for ki, (K, s) in enumerate(((96, 1), (5 * BK + 12, 3))):
            en, epi = EPILOGUES[(2 * li + ki + c) % 5]
            out.append(Case(f"tiled cfg {c} ({BM}x{BN}x{BK}) {ln} {M}x{N}x{K} splits {s} {en}", M, N, K,
                            **_tiled(c, at, bt, s), **epi))
    return out


def _scalar(name, ln, at, bt, i, M=132, N=68, K=72, **kw):
    en, epi = EPILOGUES[i % 5]
    # (PDN_GEMM_CFG is honoured on the float4 path only: here it must be ignored)
    return Case(f"scalar {name} {ln} {M}x{N}x{K} {en}", M, N, K, at=at, bt=bt, env={"PDN_GEMM_CFG": "0,1"},
                route=dict(family="tiled", cfg=5, akin=int(not at), bkin=int(bt), vec=0), **kw, **epi)


def scalar_cases():
    """gemm_f32_mfma_kernel<2, 2, 1, 1, 32, A_KIN, B_KIN, VEC = false>: each way of losing the float4 path, once per layout
    it applies to, on shapes that would otherwise keep it (132 x 68 x 72, row strides multiples of 4)."""
    out, i = [], 0
    for ln, at, bt in LAYOUTS:
        out.append(_scalar("A base 4B off", ln, at, bt, i, a_off=1))
        out.append(_scalar("B base 4B off", ln, at, bt, i + 1, b_off=1))
        out.append(_scalar("A odd row stride", ln, at, bt, i + 2, a_pad=1))
        out.append(_scalar("B odd row stride", ln, at, bt, i + 3, b_pad=1))
        out.append(_scalar("A batch stride +1" if not bt else "B batch stride +1", ln, at, bt, i + 4, nb=(1, 2),
                           gaps=((0, 1), (0, 0), (0, 0)) if not bt else ((0, 0), (0, 1), (0, 0))))
        if not at or bt:                                    # a contraction-contiguous operand, K = 4 k + 1 (row strides 76)
            out.append(_scalar("K=4k+1", ln, at, bt, i, K=73, a_pad=0 if at else 3, b_pad=3 if bt else 0))
        if at:                                              # m-contiguous A, odd M (row stride 136)
            out.append(_scalar("odd M", ln, at, bt, i + 1, M=133, a_pad=3))
        if not bt:                                          # n-contiguous B, odd N (row stride 68)
            out.append(_scalar("odd N", ln, at, bt, i + 2, N=67, b_pad=1))
        i += 1
    # a long contraction with a workspace: the library chooses the split (asserted bit-equal over two runs when > 1)
    out.append(_scalar("odd M, K=1027, workspace", "TN", True, False, 1, M=133, K=1027, a_pad=3, slabs=8))
    return out


def colsum_cases(c):
    """gemm_f32_mfma_kernel<kCfgs[c], false, false, true, COLSUM = true>: x^T g with b_colsum, overwritten and accumulated;
    three row tiles (only tile_m == 0 sums), N = 2 BN + 36 (the n0 + tid < N guard), K = 200."""
    BM, BN, BK = tile(c)
    M, N = 2 * BM + 40, 2 * BN + 36
    return [Case(f"colsum cfg {c} ({BM}x{BN}x{BK}) TN {M}x{N}x200 accumulate {acc}", M, N, 200, colsum=acc,
                 **_tiled(c, True, False), **(dict(beta=1.0) if acc else {})) for acc in (0, 1)]


def colsum_refused_cases():
    """b_colsum in a layout without the COLSUM build: PDN_EUNSUPPORTED, nothing written."""
    kw = dict(colsum=0, refuse=EUNSUPPORTED)
    return [Case("colsum refused: A row-major", 72, 68, 200, at=False, bt=False, **kw),
            Case("colsum refused: B k-contiguous", 72, 68, 200, at=True, bt=True, **kw),
            Case("colsum refused: a batch", 72, 68, 200, at=True, bt=False, nb=(1, 2), **kw),
            Case("colsum refused: A base 4B off", 72, 68, 200, at=True, bt=False, a_off=1, **kw)]


def batch_cases():
    """Batches of 2 x 3 with different batch strides per operand, and with A shared (batch stride 0), on configurations
    0, 5, 10 over two splits (slab index batch * splits + split), accumulating into C with a residual."""
    out = []
    for c, (ln, at, bt), (ln2, at2, bt2) in ((0, LAYOUTS[0], LAYOUTS[3]), (5, LAYOUTS[2], LAYOUTS[1]), (10, LAYOUTS[1], LAYOUTS[2])):
        BM, BN, BK = tile(c)
        M, N = BM + 40, BN + 36
        out.append(Case(f"batch 2x3 cfg {c} {ln} {M}x{N}x100 splits 2", M, N, 100, nb=(2, 3), beta=1.0, res=True,
                        gaps=((4, 8), (8, 12), (12, 4)), **_tiled(c, at, bt, 2)))
        out.append(Case(f"batch 2x3 shared A cfg {c} {ln2} {M}x{N}x100 splits 2", M, N, 100, nb=(2, 3), beta=1.0, res=True,
                        a_bcast=True, gaps=((0, 0), (8, 4), (4, 12)), **_tiled(c, at2, bt2, 2)))
    return out


def reduce_cases():
    """gemm_splitk_reduce_kernel behind configuration 5 over 4 splits (K = 256 = 4 x 2 k-tiles): the float4 form (N = 68 =
    ldc, everything on the 16-byte grid) and each way into the scalar form; the off-grid workspace also sends the
    partial store down the guarded epilogue."""
    def case(name, N=68, **kw):
        kw = {**FULL, **kw}
        return Case(f"reduce {name} 100x{N}x256 splits 4", 100, N, 256, **_tiled(5, False, kw.pop("bt", False), 4), **kw)
    return [case("float4"), case("float4 plain", alpha=1.0, beta=0.0, bias=False, res=False), case("scalar: ldc 69", ldc_pad=1),
            case("scalar: N 67, NT", N=67, bt=True), case("scalar: workspace 4B off", ws_off=1),
            case("scalar: bias 4B off", bias_off=1)]


def degenerate_cases():
    """K = 0 (C = bias + residual + beta C), K = 1, M = 1 / N = 1 in a batch (tiled: the skinny kernel is unbatched), and
    M, N or a batch count of 0, which write nothing."""
    t5 = {"PDN_GEMM_CFG": "5,1"}
    def r(akin, bkin, vec):
        return dict(family="tiled", cfg=5, akin=akin, bkin=bkin, vec=vec, splits=1)
    nothing = dict(writes=False, beta=1.0, bias=True)
    return [Case("K=0 NN 70x68", 70, 68, 0, bias=True, res=True, beta=2.0, env=t5, route=r(1, 0, 1)),
            Case("K=0 TN 72x68 plain", 72, 68, 0, at=True, env=t5, route=r(0, 0, 1)),
            # (K = 1: a row-major A has both strides 1 and counts as contraction-contiguous with a row stride of 1: scalar)
            Case("K=1 NN 70x68", 70, 68, 1, alpha=2.0, bias=True, env=t5, route=r(1, 0, 0)),
            Case("K=1 TN 72x68", 72, 68, 1, at=True, res=True, beta=1.0, env=t5, route=r(0, 0, 1)),
            Case("M=1 batch 3 NN 1x68x8", 1, 68, 8, nb=(1, 3), bias=True, env=t5, route=r(1, 0, 1)),
            Case("N=1 batch 3 NN 70x1x8", 70, 1, 8, nb=(3, 1), res=True, beta=1.0, env=t5, route=r(1, 1, 0)),
            Case("M=N=1 batch 2x3 NN 1x1x8", 1, 1, 8, nb=(2, 3), **FULL, env=t5, route=r(1, 1, 0)),
            Case("M=0", 0, 68, 8, **nothing), Case("N=0", 70, 0, 8, **nothing),
            Case("outer batch 0", 70, 68, 8, nb=(0, 3), **nothing), Case("inner batch 0", 70, 68, 8, nb=(2, 0), **nothing)]


def grid_limit_cases():
    """batch * splits is the grid's y extent: 255 x 257 = 65535 products of 1 x 1 x 1 run and are right; 256 x 256 = 65536
    is refused as an invalid argument (pdn_last_error names the entry) and C is untouched."""
    return [Case("65535 products 1x1x1", 1, 1, 1, nb=(255, 257), res=True, beta=1.0, alpha=2.0,
                 route=dict(family="tiled", cfg=5, akin=1, bkin=1, vec=0, splits=1)),
            Case("65536 products 1x1x1 refused", 1, 1, 1, nb=(256, 256), res=True, beta=1.0, refuse=EINVAL)]


# =====================================================================================================================
# mask epilogues at every MASKS tile shape
# =====================================================================================================================
def mask_cases(c):
    """gemm_f32_mfma_kernel<kCfgs[c], true, B_KIN, true, false, MASKS = true> behind pdn_linear_relu_fwd_f32 (W in either
    orientation) and pdn_linear_dx_masked_f32 (with / without `existing`, with / without the partials; configuration 8
    without, as the library requires).  M = 2 BM + 40 (an 8-row last band), N = 2 BN + 32, K = 84.  Integer pass: the bits
    equal z >= 0 at the frequent zeros too, h = max(0, z), masked-out dx exactly 0, the partial sums exact."""
    BM, BN, BK = tile(c)
    M, N, K = 2 * BM + 40, 2 * BN + 32, 84
    def route(bt):
        return dict(env={"PDN_GEMM_CFG": f"{c},1"}, route=dict(family="tiled", cfg=c, akin=1, bkin=int(bt), vec=1, splits=1))
    out = [Case(f"relu cfg {c} ({BM}x{BN}) W row-major {M}x{N}x{K} bias", M, N, K, entry="relu", bt=False, bias=True, **route(False)),
           Case(f"relu cfg {c} ({BM}x{BN}) W.T {M}x{N}x{K} ldh=N+4", M, N, K, entry="relu", bt=True, ldc_pad=4, **route(True))]
    seen = set()
    for bt in (True, False):
        for ex, pa in ((True, True), (False, False), (True, False), (False, True)):
            pa = pa and c != 8
            if (bt, ex, pa) in seen:
                continue
            seen.add((bt, ex, pa))
            out.append(Case(f"dx cfg {c} ({BM}x{BN}) {'W row-major' if bt else 'W.T'} {M}x{N}x{K} existing {int(ex)} partials {int(pa)}",
                            M, N, K, entry="dx", bt=bt, existing=ex, partials=pa, ldc_pad=4 if (ex and not pa) else 0, **route(bt)))
    return out


def mask_scalar_cases():
    """The scalar MASKS build (2, 2, 1, 1, 32, VEC = false): x / g 4 bytes off the 16-byte grid; PDN_GEMM_CFG is ignored."""
    kw = dict(a_off=1, env={"PDN_GEMM_CFG": "0,1"})
    def r(bt):
        return dict(family="tiled", cfg=5, akin=1, bkin=int(bt), vec=0, splits=1)
    return [Case("relu scalar x 4B off 168x160x84", 168, 160, 84, entry="relu", bias=True, route=r(False), **kw),
            Case("dx scalar g 4B off 168x160x84", 168, 160, 84, entry="dx", bt=True, existing=True, partials=True, route=r(True), **kw)]


# =====================================================================================================================
# streaming weight-gradient kernels
# =====================================================================================================================
def _shape_mn(s):
    th, tw = 32 * STREAM_SHAPES[s][0], 32 * STREAM_SHAPES[s][1]
    return 2 * th + 4, tw + 36


#                name                              M, N        routing variables                 a_off vec sshape kind
STREAM_VARIANTS = (
    ("dma<3,3>",                                   (192, 96),  {},                                    0, 1, 0, "dma"),
    ("lds<3,3,false>",                             (192, 96),  {"PDN_GEMM_STREAM_NODMA": "1"},        0, 1, 0, "lds"),
    ("lds<3,3,true>",                              (100, 200), {"PDN_GEMM_STREAM_SHAPE": "0"},        0, 1, 0, "lds-edge"),
    ("lds<5,2,true>",                              _shape_mn(1), {"PDN_GEMM_STREAM_SHAPE": "1"},      0, 1, 1, "lds-edge"),
    ("lds<2,5,true>",                              _shape_mn(2), {"PDN_GEMM_STREAM_SHAPE": "2"},      0, 1, 2, "lds-edge"),
    ("lds<4,2,true>",                              _shape_mn(3), {"PDN_GEMM_STREAM_SHAPE": "3"},      0, 1, 3, "lds-edge"),
    ("lds<2,4,true>",                              _shape_mn(4), {"PDN_GEMM_STREAM_SHAPE": "4"},      0, 1, 4, "lds-edge"),
    ("direct<3,3,false>, base 4B off",             (192, 96),  {},                                    1, 0, 0, "direct"),
    ("direct<3,3,true>, unaligned extents",        (101, 203), {},                                    0, 0, 0, "direct-edge"),
    # (the shape is pinned too: on aligned operands another tile shape, which 100 x 200 would get, has no direct form)
    ("direct<3,3,true>, aligned operands",         (100, 200), {"PDN_GEMM_STREAM_DIRECT": "1", "PDN_GEMM_STREAM_SHAPE": "0"},
                                                                                                      0, 1, 0, "direct-edge"),
)


def _stream(vec, sshape, kind, splits):
    return dict(family="stream", cfg=0, akin=0, bkin=0, vec=vec, splits=splits, sshape=sshape, kind=kind)


def stream_cases(v):
    """One streaming kernel (STREAM_VARIANTS[v]) on x^T g with K = 2048 and 2061 (a ragged last split and last wave), over
    1 split (alpha, bias, residual, beta in the kernel's own epilogue) and 3 / 5 splits (slabs + reduce), each plain and
    with alpha 0.5 + bias + residual + beta 1 into an ldc = N + 4 output."""
    name, (M, N), env, a_off, vec, sshape, kind = STREAM_VARIANTS[v]
    out = []
    for K in (2048, 2061):
        for s in (1, 3, 5):
            for en, epi in (("plain", {}), ("a.5+bias+res+b1,ldc=N+4", dict(alpha=0.5, bias=True, res=True, beta=1.0, ldc_pad=4))):
                out.append(Case(f"stream {name} {M}x{N}x{K} splits {s} {en}", M, N, K, at=True, a_off=a_off, slabs=s,
                                env={**env, "PDN_GEMM_STREAM_SPLITS": str(s)}, route=_stream(vec, sshape, kind, s), **epi))
    return out


def stream_batch_and_threshold_cases():
    """Batches of 3 (different strides per operand) and 64 are streamed, 65 go to the tiled kernel; K = 2047 is tiled,
    K = 2048 streamed (PDN_GEMM_CFG pins the tiled side and is ignored by the stream route)."""
    t5 = {"PDN_GEMM_CFG": "5,1"}
    tiled = dict(family="tiled", cfg=5, akin=0, bkin=0, vec=1, splits=1)
    return [Case("stream batch 3 dma 96x96x2048 splits 3", 96, 96, 2048, at=True, nb=(1, 3), gaps=((0, 4), (0, 8), (0, 12)),
                 slabs=3, env={"PDN_GEMM_STREAM_SPLITS": "3"}, route=_stream(1, 0, "dma", 3), res=True, beta=1.0),
            Case("stream batch 8x8 lds-edge 32x36x2048 splits 1", 32, 36, 2048, at=True, nb=(8, 8), bias=True, slabs=1,
                 env={"PDN_GEMM_STREAM_SHAPE": "0", "PDN_GEMM_STREAM_SPLITS": "1", **t5}, route=_stream(1, 0, "lds-edge", 1)),
            Case("batch 5x13 = 65 is tiled 32x36x2048", 32, 36, 2048, at=True, nb=(5, 13), bias=True, slabs=1,
                 env={"PDN_GEMM_STREAM_SHAPE": "0", "PDN_GEMM_STREAM_SPLITS": "1", **t5}, route=tiled),
            Case("K=2047 is tiled 192x96", 192, 96, 2047, at=True, slabs=1, env=t5, route=tiled),
            Case("K=2048 is streamed 192x96", 192, 96, 2048, at=True, slabs=1, env={**t5, "PDN_GEMM_STREAM_SPLITS": "1"},
                 route=_stream(1, 0, "dma", 1))]


_register("tiled_every_configuration_and_layout", tiled_cases, list(range(len(KCFGS))))
_register("scalar_staging", scalar_cases)
_register("fused_column_sums", colsum_cases, list(range(len(KCFGS))))
_register("fused_column_sums_refused", colsum_refused_cases)
_register("batches_over_two_splits", batch_cases)
_register("slab_reduce_both_forms", reduce_cases)
_register("degenerate_extents", degenerate_cases)
_register("grid_y_limit", grid_limit_cases)
_register("mask_epilogues", mask_cases, list(MASK_CFGS))
_register("mask_epilogues_scalar", mask_scalar_cases)
_register("stream_kernels", stream_cases, list(range(len(STREAM_VARIANTS))))
_register("stream_batches_and_length_threshold", stream_batch_and_threshold_cases)


# =====================================================================================================================
# the tables say what they claim (CPU)
# =====================================================================================================================
def test_tile_table_matches_the_library_source():
    """KCFGS and STREAM_SHAPES restate kCfgs / kShapes of csrc/gemm_select.h (the selector of csrc/gemm.hip)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pydynet_amd", "csrc", "gemm_select.h")).read()
    body = src[src.index("static const TileCfg kCfgs[]"):src.index("static const int kNumCfgs")]
    rows = re.findall(r"^\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), [\d.]+f\},", body, flags=re.M)
    assert tuple(tuple(int(x) for x in r) for r in rows) == KCFGS
    shapes = re.search(r"kShapes\[5\]\[2\] = \{(.*?)\};", src).group(1)
    assert tuple((int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", shapes)) == STREAM_SHAPES


def test_case_tables_cover_what_they_claim():
    """Every one of the 13 x 4 float4 instantiations is pinned by route with both contractions; every configuration meets
    all five epilogues and every layout meets each for some configuration; the four scalar layouts, the COLSUM build per
    configuration, the six MASKS shapes for both entries (with and without partials but for configuration 8), both
    splits > 1 forms of the reduce, and the ten streaming variants are each pinned at least once."""
    by_layout = {}
    for c in range(len(KCFGS)):
        cases = tiled_cases(c)
        BM, BN, BK = tile(c)
        assert {(k.route["cfg"], k.route["akin"], k.route["bkin"], k.route["vec"], k.route["splits"]) for k in cases} == \
            {(c, a, b, 1, s) for a in (0, 1) for b in (0, 1) for s in (1, 3)}
        assert all(k.M > 4 and k.N > 16 and k.N != 288 and k.K != 288 and k.K < 2048 and k.M % 4 == 0 and k.N % 4 == 0 for k in cases)
        assert all(k.M == 8 * BM + 40 and k.N == 2 * BN + 36 and k.K in (96, 5 * BK + 12) for k in cases)
        epi = lambda k: (k.alpha, k.beta, k.bias, k.res, k.ldc_pad, k.bias_off)
        assert len({epi(k) for k in cases}) == 5
        for k in cases:
            by_layout.setdefault((k.at, k.bt), set()).add(epi(k))
        assert {(k.colsum, k.route["cfg"], k.route["akin"], k.route["bkin"], k.route["vec"]) for k in colsum_cases(c)} == \
            {(0, c, 0, 0, 1), (1, c, 0, 0, 1)}
    assert len(by_layout) == 4 and all(len(v) == 5 for v in by_layout.values())
    assert {(k.route["akin"], k.route["bkin"]) for k in scalar_cases() if k.route["vec"] == 0 and k.route["cfg"] == 5} == \
        {(a, b) for a in (0, 1) for b in (0, 1)}
    for c in MASK_CFGS:
        cases = mask_cases(c)
        assert {(k.entry, k.route["bkin"]) for k in cases} == {(e, b) for e in ("relu", "dx") for b in (0, 1)}
        assert all(k.route["cfg"] == c and k.route["vec"] == 1 for k in cases)
        assert {k.partials for k in cases if k.entry == "dx"} == ({False} if c == 8 else {False, True})
        assert {k.existing for k in cases if k.entry == "dx"} == {False, True}
    assert {k.entry for k in mask_scalar_cases() if k.route["vec"] == 0} == {"relu", "dx"}
    assert all(k.route["splits"] == 4 and k.route["cfg"] == 5 for k in reduce_cases())
    kinds = [(stream_cases(v)[0].route["kind"], stream_cases(v)[0].route["sshape"], stream_cases(v)[0].route["vec"])
             for v in range(len(STREAM_VARIANTS))]
    assert len(set(kinds)) == 10 and {k[0] for k in kinds} == {"dma", "lds", "lds-edge", "direct", "direct-edge"}
    assert {k[1] for k in kinds} == {0, 1, 2, 3, 4}
    for v in range(len(STREAM_VARIANTS)):
        assert {(k.K, k.route["splits"], k.bias) for k in stream_cases(v)} == \
            {(K, s, e) for K in (2048, 2061) for s in (1, 3, 5) for e in (False, True)}


# =====================================================================================================================
# the harness notices (CPU): the emulator's pdn_gemm_f32 with one defect at a time
# =====================================================================================================================
DEFECT_CASE = Case("defect probe NN 70x68x72", 70, 68, 72, alpha=0.5, bias=True, res=True, beta=2.0, ldc_pad=4)


def _with_defect(monkeypatch, emu, defect):
    """Wrap the emulated pdn_gemm_f32 (positional arguments as in include/pdn_hip.h) with one defect."""
    from tests.abi_emulator import view, flat
    good = emu.pdn_gemm_f32
    keep = []

    def bad(M, N, K, alpha, A, a_rs, a_cs, B, b_rs, b_cs, beta, C, ldc, bias, nb1, nb2, a1, a2, b1, b2, c1, c2, residual,
            colsum, colsum_acc, ws, wsb, stream):
        if defect == "last k dropped":
            K -= 1
        if defect == "bias one column right":
            shifted = np.zeros(N + 1, F32)
            shifted[1:] = flat(bias, N)
            keep.append(shifted)
            bias = shifted.ctypes.data
        if defect == "residual ignored" and beta != 0.0:
            residual = None
        saved = []
        if defect == "bf16 operands":
            for ptr, shape, strides in ((A, (nb1, nb2, M, K), (a1, a2, a_rs, a_cs)), (B, (nb1, nb2, K, N), (b1, b2, b_rs, b_cs))):
                v = view(ptr, shape, strides, F32)
                saved.append((v, np.array(v)))
                v[...] = ref.round_bf16(saved[-1][1])
        rc = good(M, N, K, alpha, A, a_rs, a_cs, B, b_rs, b_cs, beta, C, ldc, bias, nb1, nb2, a1, a2, b1, b2, c1, c2, residual,
                  colsum, colsum_acc, ws, wsb, stream)
        for v, orig in saved:
            v[...] = orig
        if defect == "padding column written":
            assert ldc > N
            flat(C, N + 1)[N] = 7.0
        return rc

    monkeypatch.setattr(emu, "pdn_gemm_f32", bad)


def test_harness_passes_the_defect_probe_unwrapped(emulated_hip, monkeypatch, capfd):
    from pydynet_amd import _lib
    _run_case(emulated_hip, _lib.lib(), DEFECT_CASE, monkeypatch, capfd)


@pytest.mark.parametrize("defect", ["last k dropped", "bias one column right", "padding column written", "residual ignored"])
def test_harness_notices_a_defect(emulated_hip, monkeypatch, capfd, defect):
    """Both passes fail on: the last contraction index dropped, the bias applied one column to the right, a write into the
    first padding column of an ldc > N output, the residual ignored when beta != 0."""
    from pydynet_amd import _lib
    emu = _lib.lib()
    _with_defect(monkeypatch, emu, defect)
    for kind in ("exact", "precision"):
        with pytest.raises(AssertionError):
            _run_case(emulated_hip, emu, DEFECT_CASE, monkeypatch, capfd, passes=(kind,))


def test_harness_notices_bfloat16_operands_in_the_precision_pass_only(emulated_hip, monkeypatch, capfd):
    """Integers in [-4, 4] are exact in bfloat16: the exact pass cannot see operands rounded to it, the precision pass
    must -- the reason both passes exist."""
    from pydynet_amd import _lib
    emu = _lib.lib()
    _with_defect(monkeypatch, emu, "bf16 operands")
    _run_case(emulated_hip, emu, DEFECT_CASE, monkeypatch, capfd, passes=("exact",))
    with pytest.raises(AssertionError):
        _run_case(emulated_hip, emu, DEFECT_CASE, monkeypatch, capfd, passes=("precision",))
