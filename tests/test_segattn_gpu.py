"""The segmented (document-masked) resident attention kernels through the C ABI of include/pdn_segattn.h, on a real MI355X.

(1) parity with the float64 statement (pydynet_amd/core/fused/segments.py) at 1e-4 of each result's largest entry: o, lse, dq,
    dk, dv for head dims 48 / 64, L = 64 (two tiles), 256 (one full chunk), 512 (the chunked form, two chunks), document
    layouts whose boundaries fall off the 32-row tile grid, and RoPE absent, applied inside the kernels, or applied beforehand
    (`prerotated`: dq / dk still come back as gradients of the UN-rotated operands).  Launch counter slot 43 moves, with 9 / 10;
    7 and 8 (the persistent kernels) do not.
(2) isolation, bit for bit: other values in document A's q / k / v rows leave the o and lse rows of every other document as they
    were, and a d_o that is non-zero on document B's rows only leaves exact zeros in the dq / dk / dv rows of the others."""
import ctypes

import numpy as np
import pytest

from pydynet_amd import _lib
from pydynet_amd.core.fused import segments as S
from pydynet_amd.llm.llama import compute_cos_sin_cache

pytestmark = pytest.mark.gpu

B, H = 2, 3
RT = 1e-4


def ids_of(lengths, L):
    """segment ids of one row from document lengths (cut at L; what remains is one more document)"""
    seg, at, n = np.zeros(L, np.int32), 0, 0
    for n, ln in enumerate(lengths):
        seg[at:at + ln] = n
        at += ln
        if at >= L:
            return seg
    seg[at:] = n + 1
    return seg


def layout(name, L):
    offgrid = ids_of([1, 31, 33, 17, 63, 2, 45] * 8, L)
    rows = {
        "offgrid": [offgrid, offgrid],
        "single": [ids_of([L // 2 - 3, 1], L)] * 2,                # a one-token document in the middle
        "whole": [np.zeros(L, np.int32)] * 2,
        "perrow": [ids_of([5, 40, 7], L), ids_of([L - 9, 9], L)],
        "cross256": [ids_of([200, 100], L)] * 2,                   # 200 .. 299 crosses position 256
        "at256": [ids_of([90, 166, 70], L), ids_of([256], L)],     # a document that starts exactly at 256
    }[name]
    return np.stack(rows).astype(np.int32)


CASES = [(hd, L, name) for hd in (48, 64) for L in (64, 256, 512)
         for name in ("offgrid", "single", "whole", "perrow") + (("cross256", "at256") if L == 512 else ())]


def counters():
    buf = (ctypes.c_int64 * 44)()
    _lib.lib().call("pdn_kernel_counters", buf, 44, 1)
    return list(buf)


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    print(f"{what}: max err {err:.3e} of {scale:.3e}")
    assert err <= RT * scale, (what, err, scale)


def device_bounds(hip, seg):
    L = _lib.lib()
    Bn, Ln = seg.shape
    ids, start, end = hip.asarray(seg), hip.empty(seg.shape, np.int32), hip.empty(seg.shape, np.int32)
    L.call("pdns_segment_bounds_i32", ids._ptr, Bn, Ln, start._ptr, end._ptr, hip.err_flag_ptr(), hip.stream())
    return start, end


def run(hip, q, k, v, d_o, seg, cos=None, sin=None, prerotated=0):
    """o, lse, dq, dk, dv of the library for host operands (B, L, H, hd)"""
    L = _lib.lib()
    Bn, Ln, Hn, hd = q.shape
    start, end = device_bounds(hip, seg)
    qd, kd, vd, gd = (hip.asarray(np.ascontiguousarray(a, np.float32)) for a in (q, k, v, d_o))
    o, lse = hip.empty(q.shape, np.float32), hip.empty((Bn, Hn, Ln), np.float32)
    dq, dk, dv = (hip.empty(q.shape, np.float32) for _ in range(3))
    cd = hip.asarray(np.ascontiguousarray(cos, np.float32)) if cos is not None else None
    sd = hip.asarray(np.ascontiguousarray(sin, np.float32)) if sin is not None else None
    rs, bs = Hn * hd, Ln * Hn * hd
    fwd_tables = (None, None) if (prerotated or cd is None) else (cd._ptr, sd._ptr)
    L.call("pdns_attention_fwd_f32", qd._ptr, kd._ptr, vd._ptr, o._ptr, lse._ptr, Bn, Hn, Ln, hd, rs, bs, rs, bs,
           fwd_tables[0], fwd_tables[1], start._ptr, hip.stream())
    ws, wsb = hip.workspace(L.query("pdn_attention_bwd_workspace_bytes", Bn, Hn, Ln))
    L.call("pdns_attention_bwd_f32", qd._ptr, kd._ptr, vd._ptr, o._ptr, gd._ptr, lse._ptr, dq._ptr, dk._ptr, dv._ptr,
           Bn, Hn, Ln, hd, rs, bs, rs, bs, cd._ptr if cd is not None else None, sd._ptr if sd is not None else None,
           prerotated, start._ptr, end._ptr, ws, wsb, hip.stream())
    return [a.get() for a in (o, lse, dq, dk, dv)]


def operands(hd, L, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, L, H, hd)).astype(np.float32) for _ in range(4)]


@pytest.mark.parametrize("rope", ["none", "inside", "prerotated"])
@pytest.mark.parametrize("hd,L,name", CASES)
def test_kernels_match_the_float64_statement(hip, hd, L, name, rope):
    assert _lib.lib().query("pdns_attention_supported", L, hd) == 1
    seg = layout(name, L)
    q, k, v, d_o = operands(hd, L, 11)
    start, _ = S.bounds(seg)
    cos = sin = None
    if rope != "none":
        c, s = compute_cos_sin_cache(hd, L, dtype=np.float32)
        cos, sin = c.numpy(), s.numpy()
    # the statement: rotate, attend, rotate the gradients back
    qr, kr = (S.rotate(q, cos, sin), S.rotate(k, cos, sin)) if cos is not None else (q, k)
    o64, lse64, _ = S.attention_forward(qr, kr, v, start)
    dq64, dk64, dv64 = S.attention_backward(qr, kr, v, d_o, start)
    if cos is not None:
        dq64, dk64 = S.rotate(dq64, cos, sin, -1.0), S.rotate(dk64, cos, sin, -1.0)
    counters()
    if rope == "prerotated":
        got = run(hip, qr.astype(np.float32), kr.astype(np.float32), v, d_o, seg, cos, sin, prerotated=1)
    else:
        got = run(hip, q, k, v, d_o, seg, cos, sin)
    cnt = counters()
    assert cnt[43] == 2 and cnt[9] == 1 and cnt[10] == 1 and cnt[7] == 0 and cnt[8] == 0, (cnt[7:11], cnt[43])
    for g, w, what in zip(got, (o64, lse64, dq64, dk64, dv64), ("o", "lse", "dq", "dk", "dv")):
        close(g, w, f"{what} hd{hd} L{L} {name} {rope}")
    if rope == "prerotated":
        # dq / dk are gradients of the un-rotated operands: the rotated ones differ from them by far more than the tolerance
        still_rotated = S.rotate(dq64, cos, sin)
        assert np.abs(still_rotated - dq64).max() > 100 * RT * np.abs(dq64).max()


@pytest.mark.parametrize("hd,L", [(48, 256), (64, 512)])
def test_documents_are_isolated_bit_for_bit(hip, hd, L):
    seg = layout("offgrid" if L == 256 else "cross256", L)
    q, k, v, d_o = operands(hd, L, 12)
    doc = 2 if L == 256 else 1                            # document A: off the tile grid / across the chunk boundary
    in_a = seg == doc
    assert in_a.any() and not in_a.all()
    base = run(hip, q, k, v, d_o, seg)
    rng = np.random.default_rng(13)
    q2, k2, v2 = q.copy(), k.copy(), v.copy()
    for a in (q2, k2, v2):
        a[in_a] = 3.0 * rng.standard_normal((int(in_a.sum()), H, hd)).astype(np.float32)
    other = run(hip, q2, k2, v2, d_o, seg)
    assert not np.array_equal(base[0][in_a], other[0][in_a])               # document A itself did change
    assert np.array_equal(base[0][~in_a], other[0][~in_a])                 # o: (B, L, H, hd)
    lse_rows = np.broadcast_to((~in_a)[:, None, :], base[1].shape)         # lse: (B, H, L)
    assert np.array_equal(base[1][lse_rows], other[1][lse_rows])
    # a gradient that enters at document A's rows only stays there
    g = np.zeros_like(d_o)
    g[in_a] = d_o[in_a]
    _, _, dq, dk, dv = run(hip, q, k, v, g, seg)
    for a, what in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
        assert np.abs(a[in_a]).max() > 0, what
        assert (a[~in_a] == 0).all(), (what, float(np.abs(a[~in_a]).max()))
