"""`segment_ids` on the attention nodes, and the bounds kernel behind them -- emulated C ABI and (``-m gpu``) a real MI355X.

(a) pdns_segment_bounds_i32 against the statement (pydynet_amd/core/fused/segments.py): arbitrary non-decreasing ids with gaps,
    at L = 32 and L = 1024; a row that decreases raises the error flag and gets plain causal bounds;
(b) fused.attention and fused.qkv_attention with segments against the same nodes on `cpu` (which add the statement's mask), on
    the entries of include/pdn_segattn.h;
(c) a shape the segmented kernels do not take (L = 50, head dim 32): the block mask is formed on the device and the masked path
    runs -- no pdns_ attention entry, the same numbers;
(d) a host array with a decreasing row is a ValueError before anything runs; so are segments without causal / at a start_pos."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core import fused
from pydynet_amd.core.fused import segments as S
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import compute_cos_sin_cache
from tests.conftest import device_variants
from tests.test_llama_golden import close, host


def _extend():
    from tests.abi_emulator import _segattn
    _segattn.extend()                                     # (under the emulator: the pdns_ entries of include/pdn_segattn.h)


def _counters():
    buf = (ctypes.c_int64 * 44)()
    _lib.lib().call("pdn_kernel_counters", buf, 44, 1)
    return list(buf)


def _random_ids(rng, B, L):
    """non-decreasing rows with runs of random lengths and gaps between the ids"""
    steps = (rng.random((B, L)) < 0.08) * rng.integers(1, 6, (B, L))
    steps[:, 0] = rng.integers(0, 4, B)
    return np.cumsum(steps, axis=1).astype(np.int32)


def check_bounds_kernel(dev):
    _extend()
    from pydynet_amd import hipnp as hp
    L = _lib.lib()
    rng = np.random.default_rng(21)
    for Ln in (32, 1024):
        seg = _random_ids(rng, 5, Ln)
        seg[1, :] = 7                                     # one document
        seg[2, :] = np.arange(Ln) * 3                     # every position its own
        seg[3, :5] = (0, 0, 5, 5, 9)
        seg[3, 5:] = 9 + _random_ids(rng, 1, Ln - 5)[0]
        assert not S.decreasing_rows(seg).any()
        ids, start, end = hp.asarray(seg), hp.empty(seg.shape, np.int32), hp.empty(seg.shape, np.int32)
        L.call("pdns_segment_bounds_i32", ids._ptr, 5, Ln, start._ptr, end._ptr, hp.err_flag_ptr(), hp.stream())
        hp.check_index_errors()                           # nothing raised
        want = S.bounds(seg)
        assert np.array_equal(start.get(), want[0]) and np.array_equal(end.get(), want[1]), Ln
        assert (start.get()[3, :5] == (0, 0, 2, 2, 4)).all() and (end.get()[3, :4] == (2, 2, 4, 4)).all()
        # a row that decreases: the flag, and plain causal bounds for that row alone
        bad = seg.copy()
        bad[2, Ln // 2] = bad[2, Ln // 2 - 1] - 1
        ids = hp.asarray(bad)
        L.call("pdns_segment_bounds_i32", ids._ptr, 5, Ln, start._ptr, end._ptr, hp.err_flag_ptr(), hp.stream())
        with pytest.raises(IndexError):
            hp.check_index_errors()
        got_s, got_e = start.get(), end.get()
        assert (got_s[2] == 0).all() and (got_e[2] == Ln).all()
        keep = [0, 1, 3, 4]
        assert np.array_equal(got_s[keep], want[0][keep]) and np.array_equal(got_e[keep], want[1][keep])
        assert np.array_equal(S.bounds(bad)[0], got_s) and np.array_equal(S.bounds(bad)[1], got_e)


def _segments(B, L):
    seg = np.zeros((B, L), np.int32)
    seg[0, 7:] = 1
    seg[0, 7 + L // 3:] = 4
    seg[1, L // 2 + 1:] = 2
    seg[1, L - 3:] = 3
    return seg


def _attention_on(device, q, k, v, g, seg, as_device_array=False):
    Graph.clear()
    ts = [pdn.Tensor(a, dtype=np.float32, device=device, requires_grad=True) for a in (q, k, v)]
    ids = seg
    if as_device_array:
        from pydynet_amd import hipnp as hp
        ids = hp.asarray(seg.astype(np.int32))
    out = fused.attention(*ts, causal=True, segment_ids=ids)
    (out * pdn.Tensor(g, dtype=np.float32, device=device)).sum().backward()
    return out, [host(out)] + [host(t.grad) for t in ts]


def check_attention_node_with_segments(dev):
    _extend()
    rng = np.random.default_rng(22)
    B, L, H, hd = 2, 64, 3, 48
    q, k, v, g = (rng.standard_normal((B, L, H, hd)).astype(np.float32) for _ in range(4))
    seg = _segments(B, L)
    _, ref = _attention_on("cpu", q, k, v, g, seg)
    # the cpu node is the statement
    o64 = S.attention_forward(q, k, v, S.bounds(seg)[0])[0]
    close(ref[0], o64, what="cpu node against the statement")
    for as_dev in (False, True):
        _counters()
        node, got = _attention_on(dev, q, k, v, g, seg, as_dev)
        cnt = _counters()
        assert node._kind == "segmented" and cnt[43] == 2 and cnt[9] == 1 and cnt[10] == 1 and cnt[7] == cnt[8] == 0, cnt
        for a, b, what in zip(got, ref, ("o", "dq", "dk", "dv")):
            close(a, b, what=what)
    # without the segments the numbers differ: the mask is seen
    Graph.clear()
    plain = fused.attention(*[pdn.Tensor(a, dtype=np.float32, device=dev) for a in (q, k, v)], causal=True)
    assert np.abs(host(plain) - ref[0]).max() > 1e-2


def check_masked_fallback_for_other_shapes(dev):
    _extend()
    rng = np.random.default_rng(23)
    B, L, H, hd = 2, 50, 2, 32
    q, k, v, g = (rng.standard_normal((B, L, H, hd)).astype(np.float32) for _ in range(4))
    seg = _segments(B, L)
    _, ref = _attention_on("cpu", q, k, v, g, seg)
    emu = _lib.lib()
    mark = len(getattr(emu, "calls", ()))
    _counters()
    node, got = _attention_on(dev, q, k, v, g, seg)
    cnt = _counters()
    calls = list(getattr(emu, "calls", ()))[mark:]
    assert node._kind == "stream" and cnt[43] == 0 and cnt[11] == 2, (node._kind, cnt)
    if calls:
        assert [n for n in calls if n.startswith("pdns_")] == ["pdns_segment_bounds_i32"]
    for a, b, what in zip(got, ref, ("o", "dq", "dk", "dv")):
        close(a, b, what=what)
    # ... and the GEMM + softmax composition under the same mask
    saved = fused.attention.use_flash
    fused.attention.use_flash = False
    try:
        node, got = _attention_on(dev, q, k, v, g, seg)
    finally:
        fused.attention.use_flash = saved
    assert node._kind is None
    for a, b, what in zip(got, ref, ("o", "dq", "dk", "dv")):
        close(a, b, what="composition " + what)


def check_qkv_attention_node_with_segments(dev):
    _extend()
    rng = np.random.default_rng(24)
    B, L, H, hd = 2, 64, 6, 48
    D = H * hd
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    ws = [(rng.standard_normal((D, D)) / np.sqrt(D)).astype(np.float32) for _ in range(3)]
    g = rng.standard_normal((B, L, H, hd)).astype(np.float32)
    seg = _segments(B, L)
    cos, sin = compute_cos_sin_cache(hd, L, dtype=np.float32)

    def separate(device):
        Graph.clear()
        xt = pdn.Tensor(x, dtype=np.float32, device=device, requires_grad=True)
        wt = [pdn.Tensor(w, dtype=np.float32, device=device, requires_grad=True) for w in ws]
        c, s = cos.to(device), sin.to(device)
        q, k, v = ((xt @ w).reshape(B, L, H, hd) for w in wt)
        out = fused.attention(fused.rope(q, c, s), fused.rope(k, c, s), v, causal=True, segment_ids=seg)
        (out * pdn.Tensor(g, dtype=np.float32, device=device)).sum().backward()
        return [host(out), host(xt.grad)] + [host(w.grad) for w in wt]

    def one_node(min_rows):
        Graph.clear()
        xt = pdn.Tensor(x, dtype=np.float32, device=dev, requires_grad=True)
        wt = [pdn.Tensor(w, dtype=np.float32, device=dev, requires_grad=True) for w in ws]
        assert fused.qkv_attention.applicable(xt, L, hd, seg) and not fused.qkv_attention.applicable(xt, 50, hd, seg)
        saved = fused.qkv_attention.rope_min_rows
        fused.qkv_attention.rope_min_rows = min_rows
        try:
            _counters()
            out = fused.qkv_attention(xt, *wt, cos.to(dev), sin.to(dev), H, segment_ids=seg)
            (out * pdn.Tensor(g, dtype=np.float32, device=dev)).sum().backward()
            cnt = _counters()
        finally:
            fused.qkv_attention.rope_min_rows = saved
        assert cnt[43] == 2 and cnt[7] == cnt[8] == 0, cnt
        return out.rotated, [host(out), host(xt.grad)] + [host(w.grad) for w in wt]

    ref = separate("cpu")
    # RoPE inside the attention kernels, and -- rows enough for the projection's RoPE store or the in-place pre-rotation --
    # operands that arrive rotated (`prerotated`)
    for min_rows, want_rotated in ((1 << 30, False), (1, True)):
        rotated, got = one_node(min_rows)
        assert rotated == want_rotated
        for a, b, what in zip(got, ref, ("o", "dx", "dwq", "dwk", "dwv")):
            close(a, b, what=f"{what} rotated={rotated}")


def test_bad_segments_raise_before_anything_runs(emulated_hip):
    _extend()
    rng = np.random.default_rng(25)
    q, k, v = (pdn.Tensor(rng.standard_normal((2, 32, 2, 48)).astype(np.float32), device="hip:0") for _ in range(3))
    seg = np.zeros((2, 32), np.int64)
    seg[1, 10:] = 3
    seg[1, 20] = 2                                        # decreases
    emu = _lib.lib()
    for device in ("hip:0", "cpu"):
        ts = [t.to(device) for t in (q, k, v)]
        mark = len(emu.calls)
        with pytest.raises(ValueError, match="non-decreasing"):
            fused.attention(*ts, causal=True, segment_ids=seg)
        assert not [n for n in emu.calls[mark:] if "attention" in n or n.startswith("pdns_")]
    ok = np.zeros((2, 32), np.int64)
    for kw in ({"causal": False}, {"start_pos": 1}):
        with pytest.raises(ValueError, match="segment_ids"):
            fused.attention(q, k, v, segment_ids=ok, **kw)
    with pytest.raises(ValueError, match="segment_ids"):
        fused.attention(q, k, v, segment_ids=np.zeros((2, 31), np.int64))
    with pytest.raises(ValueError, match="integer"):
        fused.attention(q, k, v, segment_ids=np.zeros((2, 32), np.float32))


for _f in (check_bounds_kernel, check_attention_node_with_segments, check_masked_fallback_for_other_shapes,
           check_qkv_attention_node_with_segments):
    device_variants(globals(), _f)
