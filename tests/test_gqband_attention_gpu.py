"""Sliding-window attention over grouped heads through `fused.attention(..., window=W)` with fewer key/value heads than query
heads, on the device (csrc/attention_gqband.hip, include/pdn_gqbandattn.h), against the float64 statement of
tests/test_band_attention_gpu.py over K / V repeated per group (dk, dv summed over each group): o, dq, dk and dv of
sum(o * w), every case on the windowed shared-K/V kernels (`_kind == "gqband"`).  Bound: the project's fp32 bound,
max|got - ref| <= 1e-4 * max|ref| per tensor."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

from tests.test_band_attention_gpu import _close, _ref

pytestmark = pytest.mark.gpu

CASES = [  # B, H, Hkv, Lq, start_pos, hd, W, operands as views
    (2, 4, 2, 70, 0, 48, 40, False),     # G 2: two tiles x two heads per workgroup; ragged L; a last workgroup with idle waves
    (1, 4, 1, 96, 0, 16, 5, False),      # G 4: four heads at one tile; both edges in one key tile
    (1, 6, 2, 100, 0, 96, 33, False),    # G 3: a workgroup's units straddle two query tiles with different key ranges
    (1, 8, 1, 40, 0, 24, 1, False),      # G 8: two workgroups per tile; W = 1: o equals v[:, :, h // G], dq and dk exact zeros
    (2, 4, 2, 8, 64, 64, 20, False),     # a prefill chunk behind 64 cached keys: keys 0 .. 44 are seen by no query
    (1, 4, 1, 1, 50, 128, 16, False),    # a single query with a lower edge
    (1, 2, 1, 160, 0, 128, 33, False),   # hd 128: LDS above 64 KB, dK/dV across the 128-key seam, a second workgroup
    (2, 4, 2, 45, 19, 32, 24, True),     # k, v views into a longer cache, q a view into a packed (B, L, 3, H, hd) buffer
]


def _inputs(case):
    B, H, Hkv, Lq, start, hd, W, views = case
    rng = np.random.default_rng(sum(case[:7]))
    return [rng.standard_normal((B, n, heads, hd)).astype(np.float32)
            for n, heads in ((Lq, H), (start + Lq, Hkv), (start + Lq, Hkv), (Lq, H))]


@functools.lru_cache(maxsize=None)
def _expected(case):
    B, H, Hkv, Lq, start, hd, W, views = case
    q, k, v, w = _inputs(case)
    G, Lk = H // Hkv, start + Lq
    o, dq, dk, dv = _ref(q, np.repeat(k, G, axis=2), np.repeat(v, G, axis=2), w, start, W)
    return o, dq, dk.reshape(B, Lk, Hkv, G, hd).sum(3), dv.reshape(B, Lk, Hkv, G, hd).sum(3)


def _slot59(lib):
    buf = (ctypes.c_int64 * 60)()
    lib.call("pdn_kernel_counters", buf, 60, 1)
    return buf[59]


@functools.lru_cache(maxsize=None)
def _run(case, window="case"):
    """(`_kind`, [o, dq, dk, dv], launches counted in slot 59) of one node on the device; `window` overrides the case's."""
    import pydynet_amd as pdn
    from pydynet_amd import _lib
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    Graph.clear()
    B, H, Hkv, Lq, start, hd, W, views = case
    Lk = start + Lq
    q_np, k_np, v_np, w_np = _inputs(case)
    tensor = lambda a, grad=True: pdn.Tensor(a, dtype=np.float32, device="hip:0", requires_grad=grad)   # noqa: E731
    if views:
        wide_np = np.zeros((B, Lq, 3, H, hd), np.float32)
        wide_np[:, :, 1] = q_np
        cache_np = [np.concatenate([a, np.ones((B, 11, Hkv, hd), np.float32)], 1) for a in (k_np, v_np)]
        wide, kc, vc = tensor(wide_np), tensor(cache_np[0]), tensor(cache_np[1])
        q, k, v = wide[:, :, 1], kc[:, :Lk], vc[:, :Lk]
    else:
        q, k, v = tensor(q_np), tensor(k_np), tensor(v_np)
    _slot59(_lib.lib())
    node = fused.attention(q, k, v, causal=True, start_pos=start, window=W if window == "case" else window)
    (node * tensor(w_np, False)).sum().backward()
    grads = [wide.grad.get()[:, :, 1], kc.grad.get()[:, :Lk], vc.grad.get()[:, :Lk]] if views else \
        [t.grad.get() for t in (q, k, v)]
    return node._kind, [node.numpy()] + grads, _slot59(_lib.lib())


@pytest.mark.parametrize("case", CASES)
def test_gqband_kernels_match_float64(hip, case):
    kind, got, launches = _run(case)
    assert kind == "gqband" and launches == 2             # (the forward entry and the backward entry)
    for what, a, b in zip(("o", "dq", "dk", "dv"), got, _expected(case)):
        if b.any():
            _close(a, b, f"{case} {what}")
        else:                                 # (W = 1: the softmax of one key has no gradient -- the bound is 0)
            assert a.shape == b.shape and not a.any(), (case, what)


def test_window_of_one_returns_the_groups_v_exactly(hip):
    assert np.array_equal(_run(CASES[3])[1][0], np.repeat(_inputs(CASES[3])[2], 8, axis=2))


def test_keys_no_query_sees_get_exact_zeros(hip):
    _, (o, dq, dk, dv), _ = _run(CASES[4])
    assert not dk[:, :45].any() and not dv[:, :45].any() and dk[:, 45:].all() and dv[:, 45:].all()


def test_gqband_backward_is_deterministic(hip):
    first, second = _run(CASES[0])[1], _run.__wrapped__(CASES[0])[1]
    assert all(np.array_equal(a, b) and np.isfinite(a).all() for a, b in zip(first, second))


def test_window_past_the_sequence_is_grouped_causal_attention(hip):
    case = CASES[0]
    kind, wide, _ = _run(case, case[4] + case[3])
    plain_kind, plain, launches = _run(case, None)
    assert kind == "gqband" and plain_kind == "gqa" and launches == 0     # (no window: the parent's kernels, slot 59 still)
    for what, a, b in zip(("o", "dq", "dk", "dv"), wide, plain):
        _close(a, b, f"W >= L against window=None, {what}")


def test_gqband_header_and_exports_agree():
    from pydynet_amd import _lib
    protos = _lib.parse_header(_lib.GQBAND_HEADER_PATHS[0])
    assert len(protos) == 4 and all(n.startswith("pdnm_") for n in protos) and not set(protos) & set(_lib.parse_header())
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnm_")}
    assert exported == set(protos), exported ^ set(protos)
