"""The kernels of the graph-replayed decode step that the chained tests reach at one shape each -- the skinny product
pdn_decode_gemv_f32 with its 24 instantiations and four staging forms, the hand-off product pdn_decode_gemv_sum_f32 and
the two greedy picks (csrc/decode.hip, csrc/decode_stage.h) -- at the sizes where their tile choice, prefetch window,
row passes, staging form and index math turn, each against a plain float64 NumPy statement of the operation
(tests/decode_step_ref.py; nothing there calls this package).

Every check is a `check_*(dev)` registered through `device_variants`: it runs on the MI355X under `-m gpu` and on the NumPy
emulation of the C ABI otherwise.  Each route has EXACT cases (operands built so that every fp32 stage is exact in any
summation order: one dropped, doubled or misplaced k-term, column or row fails `np.array_equal`) and FLOAT cases
(standard-normal operands, the criterion of tests/test_decode_layer_gpu.py: max |got - ref| / max |ref| < 1e-5).  Every
output buffer starts as NaN and is larger than what the kernel may write; the rest must still be NaN afterwards."""
import functools

import numpy as np
import pytest

from tests import decode_step_ref as ref
from tests.conftest import device_variants

F32, F64 = np.float32, np.float64


def _env(dev):
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.cuda import Device
    return hp, _lib.lib(), Device(dev)


def _ints(rng, shape, lo=-3, hi=3):
    """Small integers stored as float32: every sum of a few thousand products of them is exact, and ties are everywhere."""
    return rng.integers(lo, hi + 1, shape).astype(F32)


def _rel(got, want, what):
    """The criterion of tests/test_decode_layer_gpu.py."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()), "of", got.size)
    err = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))
    assert err < 1e-5, (what, err)


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(~(np.asarray(got, F64) == np.asarray(want, F64)))
        i = tuple(bad[0])
        raise AssertionError((what, "elements off", len(bad), "of", got.size, "first at", i, float(got[i]), float(want[i])))


def _dev_rows(hp, rows, stride, off=0):
    """rows (B, w) in a NaN-filled buffer, `stride` floats between rows, starting `off` floats into it.  Returns the
    buffer (to be kept alive) and the address of row 0."""
    B, w = rows.shape
    host = np.full(B * stride + 4, np.nan, F32)
    host[off:off + B * stride].reshape(B, stride)[:, :w] = rows
    buf = hp.from_numpy(host)
    return buf, buf._ptr + 4 * off


def _weights(rng, K, N, blk_cols, exact):
    """(N / blk_cols, K + 1, blk_cols + 4) with NaN in the padding row and columns: w_row_stride > blk_cols and
    w_block_stride > K * blk_cols.  Returns the host array and (blk_cols, w_row_stride, w_block_stride)."""
    nb = N // blk_cols
    host = np.full((nb, K + 1, blk_cols + 4), np.nan, F32)
    host[:, :K, :blk_cols] = _ints(rng, (nb, K, blk_cols)) if exact else rng.standard_normal((nb, K, blk_cols))
    return host, (blk_cols, blk_cols + 4, (K + 1) * (blk_cols + 4))


@functools.lru_cache(maxsize=None)
def _shared_weights(N, kmax):
    """One integer matrix per wide N, shared by its cases (rows [:K] of it are a (K, N) matrix of the same strides), with
    its float64 copy for the reference products."""
    host, lay = _weights(np.random.default_rng(N + kmax), kmax, N, N, True)
    return host, lay, host.astype(F64)


def _launch(hp, L, Wd, lay, xptr, x_rs, B, K, N, *, norm_w=None, eps=0.0, bias=None, res=None, alias=False, act=0, ns=0,
            hd=0, tables=False):
    """One call of pdn_decode_gemv_f32.  y: (B + 1, N + 4) of NaN (y_row_stride > N; with `alias` the residual sits in y
    itself); the residual otherwise in rows N + 8 apart; the candidate tables (B + 1, tiles).  Returns the whole y buffer
    and the whole tables."""
    blk_cols, w_rs, w_bs = lay
    y_rs, keep, rptr, r_rs = N + 4, None, None, 0
    if alias:
        y0 = np.full((B + 1, y_rs), np.nan, F32)
        y0[:B, :N] = res
        Y = hp.from_numpy(y0)
        rptr, r_rs = Y._ptr, y_rs
    else:
        Y = hp.full((B + 1, y_rs), np.nan, F32)
        if res is not None:
            (keep, rptr), r_rs = _dev_rows(hp, res, N + 8), N + 8
    NW = hp.from_numpy(norm_w) if norm_w is not None else None
    BI = hp.from_numpy(bias) if bias is not None else None
    nt = ref.n_tiles(N)
    BM = hp.full((B + 1, nt), np.nan, F32) if tables else None
    BA = hp.from_numpy(np.full((B + 1, nt), -7, np.int32)) if tables else None
    L.call("pdn_decode_gemv_f32", xptr, x_rs, NW._ptr if NW is not None else None, eps, Wd._ptr, w_rs, blk_cols, w_bs,
           BI._ptr if BI is not None else None, rptr, r_rs, Y._ptr, y_rs, B, K, N, act, ns, hd,
           BM._ptr if tables else None, BA._ptr if tables else None, hp.stream())
    return Y.get(), ((BM.get(), BA.get()) if tables else None)


def _verify(y, tabs, want, B, N, exact, what):
    assert np.isnan(y[B]).all() and np.isnan(y[:B, N:]).all(), (what, "wrote outside its B x N block")
    got = y[:B, :N]
    if exact:
        _same(got, want, what)
    else:
        _rel(got, want, what)
    if tabs is not None:
        bm, ba = tabs
        assert np.isnan(bm[B]).all() and (ba[B] == -7).all(), (what, "tables: wrote past row B")
        wv, wa = ref.candidate_tables(want if exact else got.astype(F64))
        _same(bm[:B], wv, what + ("blk_max",))
        _same(ba[:B], wa, what + ("blk_arg",))


def _plain_case(hp, L, rng, Wd, lay, W64, K, N, B, i, exact=True):
    """y = x @ W (+ bias) (+ residual) with plain rows.  The options turn with the case index i: a bias on even i, the
    candidate tables on odd i and from four rows on; B = 5 and B = 8 run with `residual` aliasing y (the second pass reloads
    it in place, decode.hip `b0 == 0 ? fres : ...`), every third other case with a residual of its own."""
    x = _ints(rng, (B, K)) if exact else rng.standard_normal((B, K)).astype(F32)
    mk = (lambda s: _ints(rng, s)) if exact else (lambda s: rng.standard_normal(s).astype(F32))
    bias = mk((N,)) if i % 2 == 0 else None
    alias = B in (5, 8)
    res = mk((B, N)) if alias or i % 3 == 0 else None
    keep, xptr = _dev_rows(hp, x, K + 4)
    y, tabs = _launch(hp, L, Wd, lay, xptr, K + 4, B, K, N, bias=bias, res=res, alias=alias, tables=i % 2 == 1 or B >= 4)
    want = ref.gemv(x, [W64[j, :K, :lay[0]] for j in range(N // lay[0])], bias, res)
    _verify(y, tabs, want, B, N, exact, ("plain", N, K, B, i))


def _sweep(dev, seed, N, cases):
    """Exact plain products at one N, every (K, B) of `cases` on rows [:K] of one shared matrix, then one float case."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(seed)
    kmax = max(K for K, _ in cases)
    host, lay, W64 = _shared_weights(N, kmax)
    with device:
        Wd = hp.from_numpy(host)
        for i, (K, B) in enumerate(cases):
            if K < 64:       # fewer rows than the narrow tile has k-slices: a matrix of its own, NaN right behind row K - 1
                own, lay_k = _weights(rng, K, N, N, True)
                _plain_case(hp, L, rng, hp.from_numpy(own), lay_k, own.astype(F64), K, N, B, i)
                continue
            _plain_case(hp, L, rng, Wd, lay, W64, K, N, B, i)
        K, B = cases[-1]
        hostf, layf = _weights(rng, K, N, N, False)
        _plain_case(hp, L, rng, hp.from_numpy(hostf), layf, hostf.astype(F64), K, N, B, 1, exact=False)


def _grid(Ks, Bs):
    return [(K, B) for K in Ks for B in Bs]


# =====================================================================================================================
# 1. pdn_decode_gemv_f32: tile widths, prefetch windows, row passes, candidate tables
# =====================================================================================================================
def check_gemv_tn16_p5_edges(dev):
    """csrc/decode.hip decode_gemv_impl, N <= 4096 and K <= 320: decode_gemv_kernel<16, NB, 5, EXACT>, 64 k-slices.  EXACT
    is K in (256, 320]: K = 256 is the last K below the window, 260 / 288 / 320 sit in it (320 = 5 full steps), K = 4 and 64
    leave whole prefetch steps skipped (`i < nsteps`); at K = 4 sixty of the 64 k-slices have no row at all: their masked
    loads must stay inside W (`k < K ? k : kslice` -- they went to row `slice`, past the matrix, and 0 * whatever lay
    there was added; the K < 64 cases bring a matrix of their own with NaN right behind its last row).  N = 20: the second
    workgroup has one live column quad (`fn < N`, the table's `break`); B = 1, 2, 3 pick NB = 1, 2, 4 (B = 3: a masked fourth
    row), B = 4 a full pass, B = 5 and 8 a second pass with the residual in y.  N = 4096: 256 workgroups, the widest
    grid of this tile."""
    _sweep(dev, 201, 20, _grid((4, 64, 256, 260, 288, 320), (1, 2, 3)) + _grid((260, 288), (4, 5, 8)))
    _sweep(dev, 202, 4096, [(288, 1), (320, 2)])


def check_gemv_tn16_p12_edges(dev):
    """csrc/decode.hip decode_gemv_impl, N <= 4096 and K > 320: decode_gemv_kernel<16, NB, 12, EXACT>.  EXACT is K in
    (704, 768]; K = 324 is the first K of this route, 704 the last below the window, 772 / 1024 / 1028 / 2048 run the tail
    loop after the 12 prefetched steps (`k = slice + P * S`), 1028 and 2048 are past the staged form (K > 1024) and B = 8 at
    K = 2048 is the largest B * K the entry takes (64 KiB of staged rows)."""
    _sweep(dev, 203, 20, _grid((324, 704, 708, 768, 772, 1024, 1028, 2048), (1, 2, 3)) + _grid((768, 2048), (4, 5, 8)))
    _sweep(dev, 204, 4096, [(1028, 3)])


def check_gemv_tn32_edges(dev):
    """csrc/decode.hip decode_gemv_impl, 4096 < N <= 16384: decode_gemv_kernel<32, NB, 12, EXACT>, 32 k-slices, EXACT is K
    in (352, 384].  N = 4100 is the first N of this route: 129 workgroups, the last with one live column quad; N = 16384 the
    last N of it."""
    _sweep(dev, 205, 4100, _grid((32, 352, 356, 384, 388), (1, 2, 3)) + _grid((384, 388), (4, 5, 8)))
    _sweep(dev, 206, 16384, [(384, 2)])


def check_gemv_tn64_edges(dev):
    """csrc/decode.hip decode_gemv_impl, N > 16384: decode_gemv_kernel<64, NB, 18, EXACT>, 16 k-slices, EXACT is K in
    (272, 288].  N = 16388 is the first N of this route (257 workgroups, one live quad in the last); K = 16 is one k-step,
    292 and 580 run the tail loop."""
    _sweep(dev, 207, 16388, _grid((16, 272, 276, 288, 292, 580), (1, 2, 3)) + _grid((288, 580), (4, 5, 8)))


def check_gemv_narrow_outputs(dev):
    """csrc/decode.hip decode_gemv_kernel<16, ...>: N = 4 (one live quad in the only workgroup), 12, 16 (exactly one
    workgroup), on both prefetch depths."""
    for N in (4, 12, 16):
        _sweep(dev, 210 + N, N, _grid((64, 324), (1, 3, 8)))


# =====================================================================================================================
# 2. pdn_decode_gemv_f32: the staging forms
# =====================================================================================================================
def _norm_rows(rng, B, K, exact):
    """Exact: |x_k| = 2 with random signs and eps = 0 (mean square 4: the scale is exactly 0.5), integer norm weight."""
    if exact:
        return (2 * rng.choice([-1, 1], (B, K))).astype(F32), _ints(rng, (K,)), 0.0
    return rng.standard_normal((B, K)).astype(F32), (1 + 0.1 * rng.standard_normal(K)).astype(F32), 1e-6


def check_gemv_staging_forms(dev):
    """csrc/decode.hip decode_gemv_kernel, `if (staged) ... else for (b ...)`: the row goes through dec_stage_* when K % 4
    == 0, K <= 1024 and x is 16-byte aligned (decode_gemv_impl `sum.base = x`); else it is staged by the kernel itself --
    RMSNorm with K <= 512 keeps an element pair per thread in registers (`small`: K = 290 leaves the second element to 34
    threads, 511 to all but one; K = 288 with x moved by one float is refused by the staged form for its alignment alone),
    above that it loops (514: the first pair past `small`; 1028: the first K % 4 == 0 past the staged form; 2050).  Each
    with and without the norm weight, exact and float."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(220)
    N = 20
    forms = [(64, 0), (288, 0), (1024, 0), (290, 0), (511, 0), (288, 1), (514, 0), (1028, 0), (2050, 0)]
    with device:
        for K, off in forms:
            for exact in (True, False):
                host, lay = _weights(rng, K, N, N, exact)
                Wd, W64 = hp.from_numpy(host), host.astype(F64)
                for B in (1, 3, 7):
                    for norm in (False, True):
                        x, nw, eps = _norm_rows(rng, B, K, exact)
                        if not norm:
                            x = _ints(rng, (B, K)) if exact else x
                        bias = _ints(rng, (N,)) if exact else rng.standard_normal(N).astype(F32)
                        keep, xptr = _dev_rows(hp, x, K + 4, off)
                        y, tabs = _launch(hp, L, Wd, lay, xptr, K + 4, B, K, N, norm_w=nw if norm else None, eps=eps,
                                          bias=bias, tables=B == 7)
                        a = ref.rmsnorm(x, nw, eps) if norm else x
                        _verify(y, tabs, ref.gemv(a, [W64[0, :K, :N]], bias), B, N, exact, ("staging", K, off, B, norm))


def _swiglu_rows(rng, B, K, exact):
    """Exact: gate in {32, -128}: 1 + expf(-32) rounds to 1, so silu(32) * u = 32 u; expf(128) = inf, so silu(-128) * u is a
    zero of either sign.  `up` integer."""
    if exact:
        return np.concatenate([rng.choice([32.0, -128.0], (B, K)), _ints(rng, (B, K))], axis=1).astype(F32)
    return rng.standard_normal((B, 2 * K)).astype(F32)


def check_gemv_swiglu_rows(dev):
    """csrc/decode.hip decode_gemv_kernel `else if (act)`: act = 1, rows of packed [gate | up] with x_row_stride > 2 K (the
    `up` half is read at xr[K + k], not at a stride), K = 96 (prefetch 5), 768 (prefetch 12, EXACT) and 2048 (tail loop; with
    B = 8 the full 64 KiB of staged rows); the down projection of the five-launch step, residual in y (decode_plan.py)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(230)
    N = 36
    with device:
        for K in (96, 768, 2048):
            for exact in (True, False):
                host, lay = _weights(rng, K, N, N, exact)
                Wd, W64 = hp.from_numpy(host), host.astype(F64)
                for B in (1, 3, 8):
                    gu = _swiglu_rows(rng, B, K, exact)
                    res = _ints(rng, (B, N)) if exact else rng.standard_normal((B, N)).astype(F32)
                    keep, xptr = _dev_rows(hp, gu, 2 * K + 12)
                    y, _ = _launch(hp, L, Wd, lay, xptr, 2 * K + 12, B, K, N, res=res, alias=True, act=1)
                    a = ref.swiglu(gu, K)
                    if exact:                     # the float64 row is 32 u (1 - 1.3e-14) or -1e-53 u: correctly rounded to
                        a = a.astype(F32)         # float32 that is 32 u or a zero, and the product of THAT row is exact
                        assert np.array_equal(a, np.where(gu[:, :K] > 0, 32 * gu[:, K:], 0))
                    _verify(y, None, ref.gemv(a, [W64[0, :K, :N]], None, res), B, N, exact, ("swiglu", K, B))


# =====================================================================================================================
# 3. pdn_decode_gemv_f32 act = 2: the merge of key-range partials, hand-built and kernel-produced
# =====================================================================================================================
MERGES = [(6, 48, 1), (6, 48, 4), (4, 64, 7), (2, 128, 3), (16, 64, 8)]


def _records(rng, B, H, hd, ns, exact):
    """(B, ns, H, 4 + hd) records [m, l, NaN, NaN | sums]; with ns > 1 the last range has no keys: m = -inf, l = 0, sums 0.
    Exact: all live m of a head equal (every weight is exp(0) = 1), integer l that add up to a power of two, integer sums:
    the merged row is a multiple of 1 / sum(l) whatever the order."""
    live = ns - 1 if ns > 1 else 1
    rec = np.full((B, ns, H, 4 + hd), np.nan, F32)
    if exact:
        l = np.ones(live)
        l[0] += (1 << (live - 1).bit_length()) - live
        rec[:, :live, :, 0] = rng.integers(-3, 4, (B, 1, H))
        rec[:, :live, :, 1] = l[None, :, None]
        rec[:, :live, :, 4:] = _ints(rng, (B, live, H, hd))
    else:
        rec[:, :live, :, 0] = rng.standard_normal((B, live, H))
        rec[:, :live, :, 1] = rng.uniform(0.5, 2.0, (B, live, H))
        rec[:, :live, :, 4:] = rng.standard_normal((B, live, H, hd))
    rec[:, live:, :, 0], rec[:, live:, :, 1], rec[:, live:, :, 4:] = -np.inf, 0.0, 0.0
    return rec


def check_gemv_merge_hand_built_records(dev):
    """csrc/decode.hip decode_gemv_kernel `if (act == 2)`: the records of a row come into LDS in one round of float4 loads
    (`i < tot`, 1024 floats per round: 312 to 8704 floats here), a thread per head turns (m, l) into weights, every element
    is ns multiply-adds.  (H, hd, ns) from one range to eight, head_dim 48 / 64 / 128; x_row_stride > the records; the
    output projection of the five-launch step, residual in y.  The pad slots 2 and 3 of every record hold NaN: they are
    never read from memory.
    `poison`: the sums of row 1's range without keys are NaN instead of 0.  The merge weighs a range by w = 0, it does not
    skip it (every producer writes zeros there: DESIGN.md 4.10), so that row is lost -- but rows 0 and 2, staged through
    the same LDS before and after it, must come out bit-exact."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(240)
    with device:
        for H, hd, ns in MERGES:
            K = H * hd
            N = K if K == 288 else 20
            x_rs = ns * H * (4 + hd) + 8
            for exact in (True, False):
                host, lay = _weights(rng, K, N, N, exact)
                Wd, W64 = hp.from_numpy(host), host.astype(F64)
                for B, poison in ((1, False), (3, False), (7, False), (3, True)):
                    if poison and not (exact and ns > 1):
                        continue
                    rec = _records(rng, B, H, hd, ns, exact)
                    want_rows = ref.merge(rec)
                    if poison:
                        rec[1, ns - 1, :, 4:] = np.nan
                    res = _ints(rng, (B, N)) if exact else rng.standard_normal((B, N)).astype(F32)
                    keep, xptr = _dev_rows(hp, rec.reshape(B, -1), x_rs)
                    y, _ = _launch(hp, L, Wd, lay, xptr, x_rs, B, K, N, res=res, alias=True, act=2, ns=ns, hd=hd)
                    want = ref.gemv(want_rows, [W64[0, :K, :N]], None, res)
                    what = ("merge", H, hd, ns, B, poison)
                    if poison:
                        assert np.isnan(y[B]).all() and np.isnan(y[:B, N:]).all(), what
                        _same(y[[0, 2], :N], want[[0, 2]], what)
                    else:
                        _verify(y, None, want, B, N, exact, what)


def _attention_inputs(rng, B, H, hd, max_len):
    D = H * hd
    qkv = rng.standard_normal((B, 3 * D)).astype(F32)
    kc = rng.standard_normal((B, max_len, D)).astype(F32)
    vc = rng.standard_normal((B, max_len, D)).astype(F32)
    ang = rng.uniform(0, 6.28, (max_len, hd // 2))
    wo = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(F32)
    return qkv, kc, vc, np.cos(ang).astype(F32), np.sin(ang).astype(F32), wo


def _merge_with_gemv(hp, L, REC, rec_rs, WO, B, D, ns, hd):
    Y = hp.full((B + 1, D + 4), np.nan, F32)
    L.call("pdn_decode_gemv_f32", REC._ptr, rec_rs, None, 0.0, WO._ptr, D, D, 0, None, None, 0, Y._ptr, D + 4, B, D, D, 2, ns,
           hd, None, None, hp.stream())
    y = Y.get()
    assert np.isnan(y[B]).all() and np.isnan(y[:B, D:]).all()
    return y[:B, :D]


def _empty_ranges_are_zero(rec, T, ns, what):
    """[m, l | sums] of a range without keys: -inf, 0, zeros -- in every producer."""
    chunk = -(-T // ns)
    for sp in range(ns):
        if sp * chunk >= T:
            assert np.all(rec[sp, :, 0] == -np.inf) and np.all(rec[sp, :, 1] == 0) and np.all(rec[sp, :, 4:] == 0), \
                (what, "range", sp, "of", ns, "without keys is not [-inf, 0 | zeros]")


def check_attention_records_of_ranges_without_keys(dev):
    """csrc/decode.hip decode_attention_kernel `if (t0 >= t1)` -> decode_gemv_kernel act = 2: pdn_decode_attention_f32 at
    pos = 2 with 4 key ranges (T = 3: one key per range, the last range has none) into a records buffer full of NaN, as
    decode_plan.py's `hp.empty` may hand it over; then the merge + output projection.  The result must be finite and the
    float64 attention of the three keys: the sums of the empty range are weighed by 0, so they have to BE zeros.
    head_dim 48 and 64 (K / V rows held in registers) and 128 (the generic instantiation)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(250)
    pos, ns, max_len = 2, 4, 16
    with device:
        for B, H, hd in ((2, 6, 48), (3, 4, 64), (1, 2, 128)):
            D = H * hd
            qkv, kc, vc, cos, sin, wo = _attention_inputs(rng, B, H, hd, max_len)
            Q, KC, VC, CS, SN, WO = map(hp.from_numpy, (qkv, kc, vc, cos, sin, wo))
            rec_rs = ns * H * (4 + hd)
            REC, POS = hp.full((B, rec_rs), np.nan, F32), hp.from_numpy(np.array([pos], np.int32))
            L.call("pdn_decode_attention_f32", Q._ptr, 3 * D, CS._ptr, SN._ptr, KC._ptr, VC._ptr, REC._ptr, B, H, hd, ns,
                   max_len * D, POS._ptr, max_len, hp.stream())
            rec = REC.get().reshape(B, ns, H, 4 + hd)
            y = _merge_with_gemv(hp, L, REC, rec_rs, WO, B, D, ns, hd)
            att = np.stack([ref.attention_row(qkv[b], kc[b], vc[b], cos, sin, pos, H) for b in range(B)])
            _rel(ref.merge(rec), att, ("attention records", hd))
            _rel(y, att @ wo.astype(F64), ("attention -> merge -> Wo", hd))
            for b in range(B):
                _empty_ranges_are_zero(rec[b], pos + 1, ns, ("attention", hd, b))


def check_attention_rows_records_of_ranges_without_keys(dev):
    """csrc/decode.hip decode_attention_kernel<.., ROWS = true>: a position per row -- 0, 1 and 2 with 4 key ranges (T <=
    3: ranges without keys in every row), a later one, and stopped rows (pos < 0: computed at position 0, T = 1, three
    empty ranges) -- into a records buffer full of NaN.  The first 8 rows are merged by pdn_decode_gemv_f32 act = 2, all 12
    by pdn_decode_wide_gemm_f32 mode 3 (csrc/decode_wide.hip, the call of tests/test_serve_chunked_gpu.py; no `pos`, so the
    stopped rows are merged as well).  Both must be finite and the float64 attention of each row's keys."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(260)
    ns, max_len, B = 4, 16, 12
    pos = np.array([0, 1, 2, -1, 9, 2, -1, 1, 0, 2, -1, 5], np.int32)
    with device:
        for H, hd in ((6, 48), (4, 64)):
            D = H * hd
            qkv, kc, vc, cos, sin, wo = _attention_inputs(rng, B, H, hd, max_len)
            Q, KC, VC, CS, SN, WO = map(hp.from_numpy, (qkv, kc, vc, cos, sin, wo))
            rec_rs = ns * H * (4 + hd)
            REC, POS = hp.full((B, rec_rs), np.nan, F32), hp.from_numpy(pos)
            L.call("pdn_decode_attention_rows_f32", Q._ptr, 3 * D, CS._ptr, SN._ptr, KC._ptr, VC._ptr, REC._ptr, B, H, hd,
                   ns, max_len * D, POS._ptr, max_len, hp.stream())
            rec = REC.get().reshape(B, ns, H, 4 + hd)
            att = np.stack([ref.attention_row(qkv[b], kc[b], vc[b], cos, sin, pos[b], H) for b in range(B)])
            want = att @ wo.astype(F64)
            _rel(_merge_with_gemv(hp, L, REC, rec_rs, WO, 8, D, ns, hd), want[:8], ("rows -> gemv merge -> Wo", hd))
            assert L.query("pdn_decode_wide_supported", B, D, H, hd, 4 * D, D, max_len) == 1
            work = hp.from_numpy(np.zeros(max(4, L.query("pdn_decode_wide_work_floats", B, D, D)), F32))
            Y = hp.full((B + 1, D), np.nan, F32)
            L.call("pdn_decode_wide_gemm_f32", REC._ptr, rec_rs, 3, None, 0.0, ns, hd, WO._ptr, D, D, 0, None, Y._ptr, D, 0,
                   None, None, None, B, D, D, work._ptr, hp.stream())
            y = Y.get()
            assert np.isnan(y[B]).all()
            _rel(y[:B], want, ("rows -> wide merge -> Wo", hd))
            for b in range(B):
                _empty_ranges_are_zero(rec[b], max(int(pos[b]), 0) + 1, ns, ("attention rows", hd, b))


# =====================================================================================================================
# 4. pdn_decode_gemv_f32: column blocks, refusals
# =====================================================================================================================
def check_gemv_column_blocks(dev):
    """csrc/decode.hip decode_gemv_kernel `blk = n / blk_cols, col = n - blk * blk_cols`: W as N / blk_cols column blocks
    `w_block_stride` apart -- the packed q | k | v and gate | up layouts of decode_plan.py -- with w_row_stride > blk_cols,
    w_block_stride > K * blk_cols and y_row_stride > N, for blk_cols = N and N / 3.  N = 12 (blocks of one column quad: a
    workgroup spans all three), 72 (blocks end inside a workgroup), 864 (3 x 288: blocks end with a workgroup), 4104 and
    16392 (the 32- and 64-column tiles; 1368 and 5464 are no multiples of either).  RMSNorm rows, as q | k | v has them."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(270)
    with device:
        for N, K in ((12, 288), (72, 100), (864, 288), (4104, 100), (16392, 64)):
            for blk_cols in (N, N // 3):
                for exact in (True, False):
                    host, lay = _weights(rng, K, N, blk_cols, exact)
                    Wd, W64 = hp.from_numpy(host), host.astype(F64)
                    for B in (1, 3):
                        x, nw, eps = _norm_rows(rng, B, K, exact)
                        keep, xptr = _dev_rows(hp, x, K + 4)
                        y, tabs = _launch(hp, L, Wd, lay, xptr, K + 4, B, K, N, norm_w=nw, eps=eps, tables=B == 3)
                        want = ref.gemv(ref.rmsnorm(x, nw, eps), [W64[j, :K, :blk_cols] for j in range(N // blk_cols)])
                        _verify(y, tabs, want, B, N, exact, ("blocks", N, K, blk_cols, B))


def check_gemv_refusals(dev):
    """csrc/decode.hip decode_gemv_impl's PDN_CHECK_ARGs: more than 8 rows, rows that do not fit the 64 KiB of staging,
    column blocks that are no multiple of 4 or do not divide N, an activation together with a norm weight, a W that is not
    16-byte aligned, and a merge of more than 256 heads (a thread per head: K = 2048 at head_dim 4).  Each is an error and
    leaves y alone."""
    from pydynet_amd._lib import HipLibraryError
    hp, L, device = _env(dev)
    with device:
        X = hp.from_numpy(np.ones(9 * 4096 + 8, F32))
        W = hp.from_numpy(np.ones(2052 * 24 + 8, F32))
        NW = hp.from_numpy(np.ones(2052, F32))
        cases = {                # (B, K, N, blk_cols, norm_w, W offset in floats, act, ns, hd, x_row_stride)
            "B = 9": (9, 64, 24, 24, None, 0, 0, 0, 0, 64),
            "B * K > 16384": (8, 2052, 24, 24, None, 0, 0, 0, 0, 2052),
            "blk_cols % 4": (1, 64, 24, 6, None, 0, 0, 0, 0, 64),
            "N % blk_cols": (1, 64, 24, 16, None, 0, 0, 0, 0, 64),
            "act with norm_w": (1, 64, 24, 24, NW, 0, 1, 0, 0, 128),
            "misaligned W": (1, 64, 24, 24, None, 1, 0, 0, 0, 64),
            "H > 256 in the merge": (1, 2048, 24, 24, None, 0, 2, 1, 4, 4096),
        }
        for name, (B, K, N, bc, nw, woff, act, ns, hd, x_rs) in cases.items():
            Y = hp.full((B, N), np.nan, F32)
            with pytest.raises(HipLibraryError):
                L.call("pdn_decode_gemv_f32", X._ptr, x_rs, nw._ptr if nw is not None else None, 0.0, W._ptr + 4 * woff, 24,
                       bc, 0, None, None, 0, Y._ptr, N, B, K, N, act, ns, hd, None, None, hp.stream())
            assert np.isnan(Y.get()).all(), name
        # the neighbours that are taken: 256 heads merge (K = 1024 at head_dim 4, one range)
        rec = np.ones((1, 1, 256, 8), F32)
        R, Y = hp.from_numpy(rec), hp.full((1, 24), np.nan, F32)
        L.call("pdn_decode_gemv_f32", R._ptr, 2048, None, 0.0, W._ptr, 24, 24, 0, None, None, 0, Y._ptr, 24, 1, 1024, 24, 2, 1,
               4, None, None, hp.stream())
        _same(Y.get(), np.full((1, 24), 1024.0), "256 heads")


# =====================================================================================================================
# 5. pdn_decode_gemv_sum_f32: the hand-off
# =====================================================================================================================
def check_gemv_sum_handoff(dev):
    """csrc/decode_stage.h dec_stage_issue / dec_stage_row behind pdn_decode_gemv_sum_f32: thread = (group g, quad q) with
    nq = K / 4 quads and G = 256 / nq groups; K = 4, 12, 64, 288, 1024 give nq = 1, 3, 16, 72, 256 and G = 256, 85, 16, 3, 1
    (K = 12 and 288: 256 - G nq = 1 and 40 threads with g >= G stay idle).  A group takes DEC_PF = 8 records up front:
    n_parts = 1 (one record, 8 G - 1 clamped slots), 8 G (the prefetch exactly), 8 G + 1 (one record in the loop behind it)
    and 16 G + 3 (the loop turns twice).  parts_row_stride > n_parts * K; N = 20: two workgroups, only the first writes x_out.
    Exact: integer base and parts (x_out bit-equal); with the norm weight the base is chosen so that the SUM is +-2."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(280)
    N = 20
    with device:
        for K in (4, 12, 64, 288, 1024):
            G = 256 // (K // 4)
            for exact in (True, False):
                host, lay = _weights(rng, K, N, N, exact)
                Wd, W64 = hp.from_numpy(host), host.astype(F64)
                for i, n_parts in enumerate((1, 8 * G, 8 * G + 1, 16 * G + 3)):
                    for B in (1, 3, 8) if exact else (3,):
                        assert B * n_parts * K * 4 < 8 << 20
                        for norm in (False, True):
                            for with_out in (False, True) if exact else (True,):
                                _sum_case(hp, L, rng, Wd, lay, W64, K, N, B, n_parts, norm, with_out, exact, i)


def _sum_case(hp, L, rng, Wd, lay, W64, K, N, B, n_parts, norm, with_out, exact, i):
    if exact:
        parts = _ints(rng, (B, n_parts, K))
        base = _ints(rng, (B, K))
        nw, eps = _ints(rng, (K,)), 0.0
        if norm:
            base = ((2 * rng.choice([-1, 1], (B, K))) - parts.astype(F64).sum(1)).astype(F32)
        bias = _ints(rng, (N,)) if i % 2 else None
    else:
        parts = (rng.standard_normal((B, n_parts, K)) / np.sqrt(n_parts)).astype(F32)
        base = rng.standard_normal((B, K)).astype(F32)
        nw, eps = (1 + 0.1 * rng.standard_normal(K)).astype(F32), 1e-6
        bias = rng.standard_normal(N).astype(F32) if i % 2 else None
    kb, bptr = _dev_rows(hp, base, K + 4)
    kp, pptr = _dev_rows(hp, parts.reshape(B, -1), n_parts * K + 4)
    XO = hp.full((B + 1, K + 4), np.nan, F32) if with_out else None
    Y = hp.full((B + 1, N + 4), np.nan, F32)
    NW = hp.from_numpy(nw) if norm else None
    BI = hp.from_numpy(bias) if bias is not None else None
    nt = ref.n_tiles(N)
    BM, BA = hp.full((B + 1, nt), np.nan, F32), hp.from_numpy(np.full((B + 1, nt), -7, np.int32))
    L.call("pdn_decode_gemv_sum_f32", bptr, K + 4, pptr, n_parts, n_parts * K + 4, XO._ptr if with_out else None,
           K + 4 if with_out else 0, NW._ptr if norm else None, eps, Wd._ptr, lay[1], lay[0], lay[2],
           BI._ptr if BI is not None else None, Y._ptr, N + 4, B, K, N, BM._ptr, BA._ptr, hp.stream())
    what = ("gemv_sum", K, n_parts, B, norm, with_out)
    x = ref.handoff(base, parts)
    if with_out:
        xo = XO.get()
        assert np.isnan(xo[B]).all() and np.isnan(xo[:B, K:]).all(), (what, "x_out: wrote outside its B x K block")
        if exact:
            _same(xo[:B, :K], x, what + ("x_out",))
        else:
            _rel(xo[:B, :K], x, what + ("x_out",))
    want = ref.gemv(ref.rmsnorm(x, nw, eps) if norm else x, [W64[0, :K, :N]], bias)
    _verify(Y.get(), (BM.get(), BA.get()), want, B, N, exact, what)


# =====================================================================================================================
# 6. the greedy picks
# =====================================================================================================================
def _history(hp, steps, B):
    """The pointer-to-pointer history of tests/test_serve_gpu.py: a (steps, B) buffer and a device word with its address."""
    buf = hp.from_numpy(np.full((steps, B), -7, np.int64))
    return buf, hp.from_numpy(np.array([buf._ptr], np.int64))


def check_pick_tick(dev):
    """csrc/decode.hip decode_pick_tick_kernel<false>: one workgroup walks the rows; a thread takes candidates tid, tid +
    256, tid + 512, tid + 768 with one round of clamped loads (`min(tid + 256 u, n - 1)`: n = 1, 255, 256, 257 leave
    clamped slots that must not count), the rest in a loop (n = 1025: one candidate in it, 2004: the loop turns for most
    threads; 1024: the four rounds exactly).  Candidates come in shuffled column order with the maximum repeated, so the lower
    COLUMN has to win whatever the position of its workgroup; a row of -inf picks its first candidate's column.  With a
    history (the token goes to (*history)[*pos * B + b]), without, and without `pos`; with an embedding table of
    emb_row_stride > D the picked row is copied bit-exactly to x_next; *pos advances once per call, not per row."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(290)
    D, emb_rs, steps, p0 = 36, 40, 5, 3
    with device:
        for n in (1, 255, 256, 257, 1024, 1025, 2004):
            V = 16 * n
            emb = rng.standard_normal((V, emb_rs)).astype(F32)
            EMB = hp.from_numpy(emb)
            for B in (1, 8):
                for mode in ("history", "pos", "bare"):
                    args = np.stack([rng.permutation(V)[:n] for _ in range(B)]).astype(np.int32)
                    vals = _ints(rng, (B, n))                                  # ties everywhere
                    for b in range(B):                                         # the maximum twice more, somewhere
                        vals[b, rng.integers(0, n, 2)] = 3.0
                    if B > 1 or mode == "bare":                                # a row without a finite candidate
                        vals[B - 1], args[B - 1] = -np.inf, np.sort(args[B - 1])
                    want = ref.pick(vals, args)
                    assert not np.isinf(vals[B - 1, 0]) or want[B - 1] == args[B - 1, 0]
                    use_emb = mode != "pos"
                    VALS, ARGS = hp.from_numpy(vals), hp.from_numpy(args)
                    IDS = hp.from_numpy(np.full(B + 1, -7, np.int64))
                    POS = hp.from_numpy(np.array([p0, -7], np.int32)) if mode != "bare" else None
                    HB, HP = _history(hp, steps, B) if mode == "history" else (None, None)
                    XN = hp.full((B + 1, D), np.nan, F32)
                    L.call("pdn_decode_pick_tick_f32", VALS._ptr, ARGS._ptr, B, n, IDS._ptr, POS._ptr if POS is not None else None,
                           HP._ptr if HP is not None else None, EMB._ptr if use_emb else None, emb_rs, D,
                           XN._ptr if use_emb else None, hp.stream())
                    what = ("pick", n, B, mode)
                    ids = IDS.get()
                    _same(ids[:B], want, what)
                    assert ids[B] == -7, what
                    if POS is not None:
                        assert POS.get().tolist() == [p0 + 1, -7], what
                    if HB is not None:
                        h = HB.get()
                        assert np.array_equal(h[p0], want) and np.all(np.delete(h, p0, 0) == -7), what
                    xn = XN.get()
                    if use_emb:
                        assert np.array_equal(xn[:B], emb[want, :D]) and np.isnan(xn[B]).all(), what
                    else:
                        assert np.isnan(xn).all(), what


def check_argmax_tick(dev):
    """csrc/decode.hip decode_argmax_tick_kernel: a workgroup of 1024 threads per row, thread tid takes columns tid, tid +
    1024, ... -- V = 1 (one thread has a column), 1023, 1024, 1025 (one thread has two), 32000 (the Llama vocabulary); rows
    `row_stride` > V apart, NaN between them.  Integer logits: ties take the first index across threads and waves; the
    maximum at index 0 and at V - 1; a row of -inf and a row of NaN each pick 0; `pos` given (advanced once) and null."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(300)
    with device:
        for V in (1, 1023, 1024, 1025, 32000):
            B, rs = 7, V + 3
            z = _ints(rng, (B, V))
            z[1, 0], z[2, V - 1] = 7.0, 7.0              # a single maximum at either end
            z[3, [0, V - 1]] = 7.0                       # ... at both: the first wins
            z[4], z[5] = -np.inf, np.nan
            z[6] = rng.standard_normal(V)
            want = ref.first_argmax(z)
            assert want[1] == 0 and want[2] == V - 1 and want[3] == 0 and want[4] == 0 and want[5] == 0
            keep, zptr = _dev_rows(hp, z, rs)
            for with_pos in (True, False):
                IDS = hp.from_numpy(np.full(B + 1, -7, np.int64))
                POS = hp.from_numpy(np.array([11, -7], np.int32))
                L.call("pdn_decode_argmax_tick_f32", zptr, rs, B, V, IDS._ptr, POS._ptr if with_pos else None, hp.stream())
                ids = IDS.get()
                _same(ids[:B], want, ("argmax", V, with_pos))
                assert ids[B] == -7 and POS.get().tolist() == [12 if with_pos else 11, -7], ("argmax", V, with_pos)


for _fn in (check_gemv_tn16_p5_edges, check_gemv_tn16_p12_edges, check_gemv_tn32_edges, check_gemv_tn64_edges,
            check_gemv_narrow_outputs, check_gemv_staging_forms, check_gemv_swiglu_rows, check_gemv_merge_hand_built_records,
            check_attention_records_of_ranges_without_keys, check_attention_rows_records_of_ranges_without_keys,
            check_gemv_column_blocks, check_gemv_refusals, check_gemv_sum_handoff, check_pick_tick, check_argmax_tick):
    device_variants(globals(), _fn)
