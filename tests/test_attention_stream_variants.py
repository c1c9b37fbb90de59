"""The streaming attention kernels of csrc/attention_stream.hip (forward, dQ, dK/dV; seven head dims behind
pdn_attention_stream_fwd_f32 / pdn_attention_stream_bwd_f32) at tile, mask and stride edges, through the C ABI and -- a short
section at the end -- through the `fused.attention` node.

Every check is one `_run_case(hp, L, case)`; each GPU test (`-m gpu`) has a twin that runs the same case list on the NumPy
emulation of the C ABI (tests/abi_emulator/_attention.py): the twins check the harness, the statements of
tests/attention_stream_ref.py and the operand plumbing.  The `test_harness_notices_*` tests show that `_run_case` fails on an
entry with one defect.

Criteria, per case:
  * selection pass (exact): q = 0 and an additive mask that is 0 at ONE key pi(b, h, q) per query and -inf at every other;
    k random, v arbitrary finite float32, dO integers in [-3, 3].  Every score is exactly the mask, p exactly one-hot,
    l = 1 (exp(0) = 1, exp(-inf) = 0, the online rescale is 1 or applied to a zero accumulator): `np.array_equal` for
    o[q] == v[pi(q)], lse == 0, dv[k] == the sum of dO[q] over pi(q) = k; with v small integers too, delta = dP at the
    selected key, dS = 0 and dq == dk == 0.  pi: random | the first visible key | the diagonal min(Lk - 1, q + start) | a key
    of the LAST key tile (non-causal: the -inf branches of the online softmax run for every earlier tile).  Catches a wrong
    key row inside a tile, a wrong tile, a wrong batch / head offset, a wrong mask stride, a key past Lk or past the causal
    horizon being admitted.
  * float64 pass: standard-normal q, k, v, dO against float64 built from the float32 inputs,
    max|got - want| <= 2e-5 max|want| + 1e-7 per tensor (tests/test_attention_stream_gpu.py), printed per case (an MI355X
    run: profiles/attention_stream_variants_gpu_tests.txt).  Keys behind the causal horizon: dk = dv = 0 exactly.
  * peaked rows (q scaled by 8): the error against float64 within 4 x the error of the same composition in NumPy float32
    (the factor: another summation order, __expf against np.exp) + 1e-7 max|want|; both printed.
  * guards: every operand, output and the delta workspace (its exact byte count) in a `Buf` with guard elements; o, lse,
    dq, dk, dv prefilled with NaN; the padding columns and rows of padded strides come back bit-identical NaN; inputs,
    mask and RoPE tables come back bit-identical.
  * determinism: a multi-tile case runs twice, bit-equal.
Fully masked rows are NaN in the reference too and are not part of this suite: the case builders assert every query keeps
a visible key.

Found by this file: `test_tile_edges_*[1]` (Lq = Lk = 1), float64 pass, dq -- a tensor that is zero in exact arithmetic and
so held to an absolute 1e-7 -- came back as 4e-7 of round-off while delta = dO . o and dP = dO . v were summed in two orders;
the dQ kernel now takes both from one contraction (docstring of `tile_edge_cases`, tests/attention_stream_ref.py)."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import attention_stream_ref as ref
from tests.attention_stream_ref import Case
from tests.conftest import device_variants
from tests.test_row_kernels import Buf, _emulated, _refused

F32, F64, U32 = np.float32, np.float64, np.uint32
RTOL, ATOL = 2e-5, 1e-7                      # tests/test_attention_stream_gpu.py: _close
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
CNT_ATT_STREAM = 11                          # PDN_CNT_ATT_STREAM (csrc/common.h)
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
FWD = ("q", "k", "v", "o", "lse", "B", "H", "Lq", "Lk", "hd", "qrs", "qbs", "krs", "kbs", "causal", "start", "mask", "sb",
       "sh", "sq", "sk", "rc", "rs")
BWD = ("q", "k", "v", "o", "do", "lse", "dq", "dk", "dv", "B", "H", "Lq", "Lk", "hd", "qrs", "qbs", "krs", "kbs", "causal",
       "start", "mask", "sb", "sh", "sq", "sk", "rc", "rs", "ws", "wsb")


# =====================================================================================================================
# the harness
# =====================================================================================================================
def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(U32), np.ascontiguousarray(b).view(U32))


def _launch(hp, L, c, q, k, v, do, mask=None, rope=None, backward=True, over=None, refuse=0, writes=True):
    """One forward (and backward) call on the case's strides.  q, do: (B, Lq, H, hd); k, v: (B, Lk, H, hd); mask: None or
    (MaskLayout, compact values); rope: None or (cos, sin).  Padding of the inputs holds random data, padding of the mask
    and everything of the outputs NaN.  Returns the logical o, lse, dq, dk, dv after the guard, padding and input checks.
    `over`: ABI arguments to replace (refusals); `refuse`: the status both entries must return, nothing written."""
    fill = np.random.default_rng(7)
    qs, ks = ref.sides(c)
    host, bufs, ptr = {}, {}, {}

    def put(name, flat, off=0):
        host[name] = flat
        bufs[name] = Buf(hp, flat)
        ptr[name] = bufs[name].ptr + 4 * off

    for name, side, a in (("q", qs, q), ("do", qs, do), ("k", ks, k), ("v", ks, v)):
        flat = fill.standard_normal(side.size).astype(F32)
        side.logical(flat)[...] = a
        put(name, flat, side.off)
    for name, side in (("o", qs), ("dq", qs), ("dk", ks), ("dv", ks)):
        put(name, np.full(side.size, np.nan, F32), side.off)
    put("lse", np.full(c.B * c.H * c.Lq, np.nan, F32))
    wsb = L.query("pdn_attention_stream_bwd_workspace_bytes", c.B, c.H, c.Lq)
    assert wsb == 4 * c.B * c.H * c.Lq
    put("ws", np.full(max(wsb // 4, 1), np.nan, F32))
    margs = dict(mask=None, sb=0, sh=0, sq=0, sk=0)
    if mask is not None:
        mlay, values = mask
        flat = np.full(mlay.size, np.nan, F32)
        mlay.logical(flat)[...] = values
        put("mask", flat, mlay.off)
        margs = dict(mask=ptr["mask"], **dict(zip(("sb", "sh", "sq", "sk"), mlay.strides)))
    rargs = dict(rc=None, rs=None)
    if rope is not None:
        put("rc", np.ascontiguousarray(rope[0]).ravel())
        put("rs", np.ascontiguousarray(rope[1]).ravel())
        rargs = dict(rc=ptr["rc"], rs=ptr["rs"])
    P = dict(ptr, B=c.B, H=c.H, Lq=c.Lq, Lk=c.Lk, hd=c.hd, qrs=qs.rs, qbs=0 if c.bs0 else qs.bs, krs=ks.rs,
             kbs=0 if c.bs0 else ks.bs, causal=c.causal, start=c.start, wsb=wsb, **margs, **rargs)
    for key, value in (over or {}).items():
        P[key] = P[key] + 4 if value == "+4" else value                             # ("+4": that pointer 4 bytes on)
    for name, keys in (("pdn_attention_stream_fwd_f32", FWD), ("pdn_attention_stream_bwd_f32", BWD)):
        if name.endswith("bwd_f32") and not backward:
            continue
        if name.endswith("fwd_f32") and refuse == EWORKSPACE:
            continue
        args = [P[key] for key in keys] + [hp.stream()]
        if refuse:
            _refused(L, refuse, name, *args)
        else:
            L.call(name, *args)
        if name.endswith("fwd_f32"):
            o_fwd = bufs["o"].get().copy()
    got = {name: bufs[name].get() for name in OUTPUTS}                              # (Buf.get checks the guard elements)
    bufs["ws"].get()
    for name in ("q", "k", "v", "do", "mask", "rc", "rs"):
        assert name not in bufs or _same_bits(bufs[name].get(), host[name]), (c.name, name, "an input changed")
    if refuse or not writes:
        for name in OUTPUTS + ("ws",):
            assert _same_bits(bufs[name].get(), host[name]), (c.name, name, "written by a call that must write nothing")
        return None
    assert _same_bits(got["o"], o_fwd), (c.name, "the backward changed o")
    out = {}
    for name, side in (("o", qs), ("dq", qs), ("dk", ks), ("dv", ks)):
        inside = np.zeros(side.size, bool)
        side.logical(inside)[...] = True
        assert _same_bits(got[name][~inside], host[name][~inside]), (c.name, name, "padding columns or rows changed")
        out[name] = np.array(side.logical(got[name]))
    out["lse"] = got["lse"].reshape(c.B, c.H, c.Lq)
    if not backward:
        for name in ("dq", "dk", "dv", "ws"):
            assert _same_bits(bufs[name].get(), host[name]), (c.name, name, "written by the forward")
    return out


def _exact(c, what, got, want):
    assert got.shape == want.shape, (c.name, what, got.shape, want.shape)
    if not np.array_equal(got.astype(F64), want):
        bad = np.argwhere(~(got.astype(F64) == want))
        i = tuple(bad[0])
        raise AssertionError((c.name, what, "not exact", len(bad), "elements, first at", i, float(got[i]), float(want[i])))


def _behind_the_horizon(c, what, got):
    """Keys no query can see under the causal flag get exactly zero gradients."""
    if c.causal and c.Lq - 1 + c.start + 1 < c.Lk:
        for name in ("dk", "dv"):
            assert np.all(got[name][:, c.Lq + c.start:] == 0.0), (c.name, what, name, "behind the horizon is not exactly 0")


def _inputs(c, rng):
    q, do = (rng.standard_normal((c.B, c.Lq, c.H, c.hd)).astype(F32) for _ in range(2))
    k, v = (rng.standard_normal((c.B, c.Lk, c.H, c.hd)).astype(F32) for _ in range(2))
    return q, k, v, do


def _rope(c):
    return ref.rope_tables(max(c.Lq, c.Lk), c.hd) if c.rope else None


def _selection_pass(hp, L, c, rng):
    m = ref.mask_values(c, rng)
    vis = ref.visible(c, m, zero_only=True)
    lay = ref.mask_layout(c.mask or "BHQK", c.B, c.H, c.Lq, c.Lk)
    ints = lambda n: rng.integers(-3, 4, (c.B, n, c.H, c.hd)).astype(F32)
    for mode in ref.PI_MODES:
        if mode == "last tile" and c.causal:
            continue
        what = f"selection, pi {mode}"
        pi = ref.choose_pi(c, mode, vis, lay.shape, rng)
        sel = (lay, ref.selection_mask(pi, lay.shape, c.Lk, m))
        q = np.zeros((c.B, c.Lq, c.H, c.hd), F32)
        k = rng.standard_normal((c.B, c.Lk, c.H, c.hd)).astype(F32)
        do = ints(c.Lq)
        v = (100.0 * rng.standard_normal((c.B, c.Lk, c.H, c.hd))).astype(F32)      # arbitrary v: the forward
        got = _launch(hp, L, c, q, k, v, do, sel, _rope(c), backward=False)
        want = ref.selection(pi, v, do)
        _exact(c, what + ": o", got["o"], want[0])
        _exact(c, what + ": lse", got["lse"], want[1])
        v = ints(c.Lk)                                                             # integer v: everything
        got = _launch(hp, L, c, q, k, v, do, sel, _rope(c))
        for name, w in zip(OUTPUTS, ref.selection(pi, v, do)):
            _exact(c, f"{what}: {name}", got[name], w)
        _behind_the_horizon(c, what, got)


def _float_pass(hp, L, c, rng, peaked):
    m = ref.mask_values(c, rng)
    ref.visible(c, m)
    mask = None if m is None else (ref.mask_layout(c.mask, c.B, c.H, c.Lq, c.Lk), m)
    q, k, v, do = _inputs(c, rng)
    q = (q * F32(c.qscale)).astype(F32)
    cos, sin = _rope(c) or (None, None)
    want = ref.attention(q, k, v, do, c.causal, c.start, m, cos, sin)
    got = _launch(hp, L, c, q, k, v, do, mask, _rope(c))
    same32 = ref.attention(q, k, v, do, c.causal, c.start, m, cos, sin, dtype=F32) if peaked else None
    for i, name in enumerate(OUTPUTS):
        g, w = got[name].astype(F64), want[i]
        assert g.shape == w.shape and np.isfinite(w).all() and np.isfinite(g).all(), (c.name, name, "shape or not finite")
        err, scale = float(np.abs(g - w).max()), float(np.abs(w).max())
        if peaked:
            own = float(np.abs(same32[i].astype(F64) - w).max())
            print(f"{c.name} | {name}: kernel err {err:.3e}, float32 statement err {own:.3e}, of {scale:.3e}")
            assert err <= 4.0 * own + 1e-7 * scale, (c.name, name, err, own, scale)
        else:
            print(f"{c.name} | {name}: err {err:.3e} of {scale:.3e} (rel {err / max(scale, 1e-30):.3e})")
            assert err <= RTOL * scale + ATOL, (c.name, name, err, scale)
    _behind_the_horizon(c, "float64", got)
    if c.twice:
        again = _launch(hp, L, c, q, k, v, do, mask, _rope(c))
        for name in OUTPUTS:
            assert _same_bits(again[name], got[name]), (c.name, name, "two runs differ")


def _run_case(hp, L, case, passes=None):
    """One case through its passes (selection: every pi; float64; peaked)."""
    assert case.B * case.H <= 6 and (max(case.Lq, case.Lk) <= 300 or (case.Lq, case.Lk, case.hd) == (513, 513, 96)), case.name
    for kind in passes or case.passes:
        rng = np.random.default_rng(zlib.crc32(case.name.encode()) + len(kind))
        if kind == "selection":
            _selection_pass(hp, L, case, rng)
        else:
            assert kind in ("float64", "peaked"), kind
            _float_pass(hp, L, case, rng, kind == "peaked")


def _register(name, make_cases, values=None):
    """`test_<name>_gpu` (marked gpu) and its twin `test_<name>_emulated` over make_cases([value])."""
    def run(hp, *v):
        from pydynet_amd import _lib
        L = _lib.lib()
        cases = make_cases(*v)
        assert cases and len({c.name for c in cases}) == len(cases)
        failed = []
        for case in cases:                               # (every case runs: one that fails does not hide the next)
            try:
                _run_case(hp, L, case)
            except AssertionError as e:
                failed.append(e)
        if failed:
            raise AssertionError(failed)

    if values is None:
        @pytest.mark.gpu
        def on_gpu(hip):
            run(hip)

        def on_emulator(emulated_hip):
            run(emulated_hip)
    else:
        @pytest.mark.gpu
        @pytest.mark.parametrize("v", values)
        def on_gpu(hip, v):
            run(hip, v)

        @pytest.mark.parametrize("v", values)
        def on_emulator(emulated_hip, v):
            run(emulated_hip, v)
    on_gpu.__doc__ = on_emulator.__doc__ = make_cases.__doc__
    globals()[f"test_{name}_gpu"] = on_gpu
    globals()[f"test_{name}_emulated"] = on_emulator


_register("tile_edges", ref.tile_edge_cases, list(ref.EDGE_LENGTHS))
_register("tile_edges_unequal_lengths_and_long_anchor", ref.unequal_edge_cases)
_register("head_dims", ref.head_dim_cases, list(ref.HEAD_DIMS))
_register("start_positions", ref.start_cases, list(ref.STARTS))
_register("mask_layouts", ref.mask_cases)
_register("strides", ref.stride_cases)
_register("rope_in_the_loads", ref.rope_cases)
_register("peaked_rows", ref.peaked_cases)


# =====================================================================================================================
# refusals
# =====================================================================================================================
def _check_refusals(hp, L):
    c = Case("refusal probe", 1, 2, 5, 9, 32, causal=1, start=4)
    rng = np.random.default_rng(11)
    q, k, v, do = _inputs(c, rng)
    cos, sin = ref.rope_tables(9, 32)
    base = _launch(hp, L, c, q, k, v, do)                                           # the probe itself is served
    assert np.isfinite(base["dk"]).all()
    D = c.H * c.hd
    tables = Buf(hp, np.concatenate([cos.ravel(), sin.ravel()]))
    rc, rs = tables.ptr, tables.ptr + 4 * cos.size
    for what, over, code in (
            ("head dim 40", dict(hd=40), EUNSUPPORTED),
            ("q row stride not divisible by 4", dict(qrs=D + 2), EINVAL),
            ("kv batch stride not divisible by 4", dict(kbs=9 * D + 2), EINVAL),
            ("RoPE: cos without sin", dict(start=0, rc=rc), EINVAL),
            ("RoPE: sin without cos", dict(start=0, rs=rs), EINVAL),
            ("RoPE with start_pos 1", dict(start=1, rc=rc, rs=rs), EUNSUPPORTED),
            ("workspace one byte short", dict(wsb=4 * c.B * c.H * c.Lq - 1), EWORKSPACE),
            ("Lk 0", dict(Lk=0), EINVAL),
            ("B H = 65536 x 1 past the grid's y limit", dict(B=65536, H=1), EUNSUPPORTED),
            ("B H = 256 x 256 past the grid's y limit", dict(B=256, H=256), EUNSUPPORTED)):
        assert _launch(hp, L, Case(what, 1, 2, 5, 9, 32, causal=1, start=4), q, k, v, do, over=over, refuse=code) is None
    for name in ("q", "k", "v"):                                                    # an operand 4 bytes off the 16-byte grid
        probe = Case(f"{name} 4 bytes off the 16-byte grid", 1, 2, 5, 9, 32, causal=1, start=4)
        assert _launch(hp, L, probe, q, k, v, do, over={name: "+4"}, refuse=EINVAL) is None
    for what, over in (("B 0", dict(B=0)), ("H 0", dict(H=0)), ("Lq 0", dict(Lq=0))):   # return 0, write nothing
        assert _launch(hp, L, Case(what, 1, 2, 5, 9, 32, causal=1, start=4), q, k, v, do, over=over, writes=False) is None
    tables.get()


def check_refusals(dev):
    """What both entries refuse on the host, each with NaN-prefilled outputs that stay untouched: an unsupported head dim,
    strides off the float4 grid, a misaligned operand, half a RoPE pair, RoPE with a start position, a short workspace,
    no keys, B H past the grid's y limit (65535; nothing oversized is launched); empty B / H / Lq return 0."""
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.cuda import Device
    with Device(dev):
        _check_refusals(hp, _lib.lib())


device_variants(globals(), check_refusals)


# =====================================================================================================================
# the harness notices (CPU): the emulated entries with one defect at a time
# =====================================================================================================================
DEFECT_CASE = Case("defect probe", 2, 3, 70, 100, 32, causal=1, start=30, mask="BHQK", q_pad=8, q_gap=2, kv_gap=3)
DEFECTS = ("key shifted by one inside the last tile", "mask head stride ignored", "causal horizon one short",
           "one row written past Lq", "padding column written", "dv missing the last query tile")


def _aligned(n):
    raw = np.zeros(n + 4, F32)
    skip = (-raw.ctypes.data % 16) // 4
    return raw, raw.ctypes.data + 4 * skip


def _with_defect(monkeypatch, emu, defect):
    """Wrap the emulated entries (positional arguments as in include/pdn_hip.h) with one defect."""
    from tests.abi_emulator import view, flat
    fwd, bwd = emu.pdn_attention_stream_fwd_f32, emu.pdn_attention_stream_bwd_f32

    def damage(a):
        """(arguments by name) -> restore(): what is done to the inputs of either entry."""
        saved = []
        if defect == DEFECTS[0]:
            t0 = 32 * ((a["Lk"] - 1) // 32)
            assert a["Lk"] - t0 >= 2
            for p in (a["k"], a["v"]):
                w = view(p, (a["B"], a["Lk"], a["H"], a["hd"]), (a["kbs"], a["krs"], a["hd"], 1), F32)
                saved.append((w, np.array(w)))
                w[:, t0:] = np.roll(saved[-1][1][:, t0:], 1, axis=1)
        if defect == DEFECTS[1]:
            assert a["mask"] and a["sh"]
            a["sh"] = 0
        if defect == DEFECTS[2]:
            assert a["causal"] and a["start"] >= 1
            a["start"] -= 1
        return saved

    def bad_fwd(*args):
        a = dict(zip(FWD, args))
        saved = damage(a)
        with np.errstate(all="ignore"):
            rc = fwd(*[a[key] for key in FWD], args[-1])
        for w, orig in saved:
            w[...] = orig
        D = a["H"] * a["hd"]
        if defect == DEFECTS[3]:
            view(a["o"], (a["B"], a["Lq"] + 1, a["H"], a["hd"]), (a["qbs"], a["qrs"], a["hd"], 1), F32)[0, a["Lq"], 0, 0] = 7.0
        if defect == DEFECTS[4]:
            assert a["qrs"] > D
            flat(a["o"], D + 1)[D] = 7.0
        return rc

    def bad_bwd(*args):
        a = dict(zip(BWD, args))
        saved = damage(a)
        with np.errstate(all="ignore"):
            rc = bwd(*[a[key] for key in BWD], args[-1])
            if defect == DEFECTS[5]:                     # dv again from the queries in front of the last query tile
                cut = 32 * ((a["Lq"] - 1) // 32)
                assert cut >= 1
                B, H, Lq = a["B"], a["H"], a["Lq"]
                keep = [_aligned(B * max(a["qbs"], Lq * a["qrs"])), _aligned(B * max(a["kbs"], a["Lk"] * a["krs"])),
                        _aligned(B * H * cut)]
                flat(keep[2][1], B * H * cut).reshape(B, H, cut)[...] = flat(a["lse"], B * H * Lq).reshape(B, H, Lq)[:, :, :cut]
                b = dict(a, Lq=cut, dq=keep[0][1], dk=keep[1][1], lse=keep[2][1])
                rc = rc or bwd(*[b[key] for key in BWD], args[-1])
        for w, orig in saved:
            w[...] = orig
        return rc

    monkeypatch.setattr(emu, "pdn_attention_stream_fwd_f32", bad_fwd)
    monkeypatch.setattr(emu, "pdn_attention_stream_bwd_f32", bad_bwd)


def test_harness_passes_the_defect_probe_unwrapped(emulated_hip):
    from pydynet_amd import _lib
    _run_case(emulated_hip, _lib.lib(), DEFECT_CASE)


@pytest.mark.parametrize("defect", DEFECTS)
def test_harness_notices_a_defect(emulated_hip, monkeypatch, defect):
    """Both passes fail on each of: the key index shifted by one inside the last key tile, the mask's head stride ignored,
    the causal horizon taken as q + start - 1, one row written past Lq, one value written into a row-stride padding column,
    dv missing the last query tile."""
    from pydynet_amd import _lib
    emu = _lib.lib()
    _with_defect(monkeypatch, emu, defect)
    for kind in ("selection", "float64"):
        with pytest.raises(AssertionError):
            _run_case(emulated_hip, emu, DEFECT_CASE, passes=(kind,))


def test_case_tables_cover_what_the_suite_claims():
    """Every length beside a tile and a workgroup edge, both causal settings; the seven head dims; the start positions off
    and on the tile grid with one and two workgroups of queries and the three key counts; every mask layout; all cases small
    and every name unique; every case's float64 mask keeps a visible key in every row."""
    cases = ref.all_cases()
    assert len({c.name for c in cases}) == len(cases)
    edges = [c for n in ref.EDGE_LENGTHS for c in ref.tile_edge_cases(n)] + ref.unequal_edge_cases()
    assert {(c.Lq, c.causal) for c in edges if c.Lq == c.Lk and c.hd == 32} == {(n, z) for n in ref.EDGE_LENGTHS for z in (0, 1)}
    assert {(c.Lq, c.Lk) for c in edges if c.Lq != c.Lk} == {(33, 129), (129, 33), (1, 300), (160, 31)}
    assert [c for c in cases if max(c.Lq, c.Lk) > 300] == [c for c in cases if (c.Lq, c.Lk, c.hd) == (513, 513, 96)] and \
        sum(max(c.Lq, c.Lk) > 300 for c in cases) == 1
    assert all(c.B * c.H <= 6 for c in cases)
    for hd in ref.HEAD_DIMS:
        assert {(c.Lq, c.Lk, c.causal, c.hd) for c in ref.head_dim_cases(hd)} == {(129, 161, 0, hd), (161, 161, 1, hd)}
    starts = [c for s in ref.STARTS for c in ref.start_cases(s)]
    assert {(c.start, c.Lq, c.Lk - c.start - c.Lq) for c in starts} == \
        {(s, n, e) for s in ref.STARTS for n in ref.START_LQ for e in (0, 40, -5) if s + n + e > 0}
    assert all(c.causal and c.hd in (24, 48) for c in starts) and 3 * sum(c.hd == 24 for c in starts) >= len(starts) - 2
    assert {c.mask for c in ref.mask_cases()} == set(ref.MASK_DIMS)
    assert {(c.Lq, c.hd) for c in ref.rope_cases()} == {(n, hd) for n in (33, 161) for hd in (24, 48, 128)}
    assert len(ref.peaked_cases()) == 2 and all(c.qscale == 8.0 for c in ref.peaked_cases())
    assert all("selection" in c.passes for c in cases if c.content != "normal" and c.qscale == 1.0)
    for c in cases:
        ref.visible(c, ref.mask_values(c, np.random.default_rng(0)))


# =====================================================================================================================
# node level: fused.attention against float64
# =====================================================================================================================
def _counters():
    from pydynet_amd import _lib
    buf = (ctypes.c_int64 * 16)()
    _lib.lib().call("pdn_kernel_counters", buf, 16, 1)
    return list(buf)


def _close(what, got, want):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"node {what}: err {err:.3e} of {scale:.3e}")
    assert err <= RTOL * scale + ATOL, (what, err, scale)


def _node(what, B, H, Lq, Lk, hd, causal, start=0, mask=None, packed_q=False, cache=0, segments=None):
    """One `fused.attention` node, forward and backward of sum(node * w), against the float64 statement: `_kind` is
    "stream" and the stream launch counter moves by two."""
    import pydynet_amd as pdn
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    Graph.clear()
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    D = H * hd
    tensor = lambda a, grad=True: pdn.Tensor(a, dtype=np.float32, device="hip:0", requires_grad=grad)
    q_np, k_np, v_np, w_np = _inputs(Case(what, B, H, Lq, Lk, hd), rng)
    if packed_q:                                         # q is a column block of a wider projection: the _q_used copy
        wide_np = rng.standard_normal((B, Lq, 3 * D)).astype(F32)
        wide = tensor(wide_np)
        q = pdn.split(wide, 3, -1)[1].reshape(B, Lq, H, hd)
        q_np = wide_np[..., D:2 * D].reshape(B, Lq, H, hd)
    else:
        q = tensor(q_np)
    if cache:                                            # k, v are slices of a longer cache
        kc_np, vc_np = (rng.standard_normal((B, Lk + cache, H, hd)).astype(F32) for _ in range(2))
        kc, vc = tensor(kc_np), tensor(vc_np)
        k, v = kc[:, :Lk], vc[:, :Lk]
        k_np, v_np = kc_np[:, :Lk], vc_np[:, :Lk]
    else:
        k, v = tensor(k_np), tensor(v_np)
    m = mask
    if segments is not None:                             # the block mask of the documents: keys from the query's own on
        from pydynet_amd import _lib
        if _emulated(_lib.lib()):                        # (under the emulator: the pdns_ entries of include/pdn_segattn.h)
            from tests.abi_emulator import _segattn
            _segattn.extend()
        first = np.array([[np.flatnonzero(row == s)[0] for s in row] for row in segments])
        m = np.where(np.arange(Lk)[None, None, None, :] >= first[:, None, :, None], 0.0, -np.inf)
    want = ref.attention(q_np, k_np, v_np, w_np, int(causal), start, m)
    _counters()
    node = fused.attention(q, k, v, causal=causal, start_pos=start, mask=mask, segment_ids=segments)
    (node * tensor(w_np, False)).sum().backward()
    assert node._kind == "stream", (what, node._kind)
    assert _counters()[CNT_ATT_STREAM] == 2, what
    assert packed_q == (node._q_used is not q.data), (what, "the q copy path")
    _close(what + " o", node.numpy(), want[0])
    if packed_q:
        g = wide.grad.get()
        _close(what + " dq", g[..., D:2 * D].reshape(B, Lq, H, hd), want[2])
        assert not g[..., :D].any() and not g[..., 2 * D:].any(), what
    else:
        _close(what + " dq", q.grad.get(), want[2])
    for name, t, w in (("dk", kc if cache else k, want[3]), ("dv", vc if cache else v, want[4])):
        g = t.grad.get()
        _close(f"{what} {name}", g[:, :Lk], w)
        assert not g[:, Lk:].any(), (what, name, "rows of the cache behind the slice got a gradient")


def check_node_takes_the_stream_kernels(dev):
    """`fused.attention` on shapes and masks only the streaming kernels serve: a full (B, H, L, Lk) mask, a (1, H, 1, Lk)
    mask, a non-contiguous q view, k / v sliced from a longer cache with start_pos 33, B = 1, and `segment_ids` at hd 32
    (the block-mask fallback)."""
    rng = np.random.default_rng(3)

    def holes(shape):
        m = np.where(rng.random(shape) < 0.3, -np.inf, 0.0).astype(F32)
        m[..., 0] = 0.0                                  # no fully masked row
        return m
    _node("full mask", 2, 3, 40, 57, 64, False, mask=holes((2, 3, 40, 57)))
    _node("(1, H, 1, Lk) mask", 2, 3, 40, 57, 64, False, mask=holes((1, 3, 1, 57)))
    _node("non-contiguous q", 2, 2, 40, 57, 32, False, packed_q=True)
    _node("cache slices, start 33", 2, 2, 40, 73, 48, True, start=33, cache=20)
    _node("B 1", 1, 3, 50, 50, 64, True)
    ids = np.sort(rng.integers(0, 4, (2, 70)), axis=1)
    _node("segment_ids at hd 32", 2, 2, 70, 70, 32, True, segments=ids)


device_variants(globals(), check_node_takes_the_stream_kernels)


def test_node_leaves_a_batch_past_the_grid_limit_to_the_composition(emulated_hip):
    """B H is the grid's y extent of the streaming kernels (65535): `_attn_kernel` picks them up to that batch and the GEMM +
    softmax composition beyond it.  The selection only: nothing is launched."""
    from pydynet_amd.core.fused import attn
    layouts = ((32, 5 * 32), (32, 9 * 32), (32, 9 * 32))
    assert attn._attn_kernel(65535, 1, 32, 5, 9, 0, None, layouts) == ("stream", None)
    assert attn._attn_kernel(65536, 1, 32, 5, 9, 0, None, layouts) == (None, None)
    assert attn._attn_kernel(256, 256, 32, 5, 9, 0, None, layouts) == (None, None)
