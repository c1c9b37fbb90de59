"""Sliding-window attention through `fused.attention(..., window=W)` on the device (csrc/attention_band.hip,
include/pdn_bandattn.h) against a float64 NumPy statement written here: o, dq, dk and dv of sum(o * w), every case on the
band kernels (`_kind == "band"`).  Bound: the project's fp32 bound, max|got - ref| <= 1e-4 * max|ref| per tensor."""
import functools
import math
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [  # B, H, Lq, start_pos, hd, W, operands as views
    (2, 3, 70, 0, 48, 40, False),     # ragged L, W no tile multiple: the band spans three key tiles
    (1, 2, 96, 0, 64, 5, False),      # W < 32: the lower edge and the diagonal in the same tile
    (1, 2, 64, 0, 48, 1, False),      # self only: o equals v exactly
    (1, 2, 64, 0, 64, 1000, False),   # W >= L: plain causal attention
    (2, 2, 8, 64, 48, 20, False),     # a prefill chunk behind 64 cached keys: keys 0 .. 44 are seen by no query
    (1, 1, 1, 50, 128, 16, False),    # a single query with a lower edge
    (1, 2, 160, 0, 128, 33, False),   # hd 128, W one past a tile, a second workgroup with an idle wave, dK/dV across the seam
    (2, 2, 45, 19, 32, 24, True),     # k, v views into a longer cache, q a view into a packed (B, L, 3, H, hd) buffer
]


def _ref(q, k, v, w, start, W):
    hd = q.shape[-1]
    Q, K, V, DO = (a.astype(np.float64).transpose(0, 2, 1, 3) for a in (q, k, v, w))
    pos, keys = np.arange(q.shape[1])[:, None] + start, np.arange(k.shape[1])[None, :]
    s = np.where((keys > pos) | (keys < pos - W + 1), -np.inf, Q @ K.swapaxes(-1, -2) / math.sqrt(hd))
    e = np.exp(s - s.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    dp = DO @ V.swapaxes(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True)) / math.sqrt(hd)
    return [a.transpose(0, 2, 1, 3) for a in (p @ V, ds @ K, ds.swapaxes(-1, -2) @ Q, p.swapaxes(-1, -2) @ DO)]


def _inputs(case):
    B, H, Lq, start, hd, W, views = case
    rng = np.random.default_rng(sum(case[:6]))
    return [rng.standard_normal((B, n, H, hd)).astype(np.float32) for n in (Lq, start + Lq, start + Lq, Lq)]


@functools.lru_cache(maxsize=None)
def _run(case, window="case"):
    """(`_kind`, [o, dq, dk, dv]) of one node on the device; `window` overrides the case's."""
    import pydynet_amd as pdn
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    Graph.clear()
    B, H, Lq, start, hd, W, views = case
    Lk = start + Lq
    q_np, k_np, v_np, w_np = _inputs(case)
    tensor = lambda a, grad=True: pdn.Tensor(a, dtype=np.float32, device="hip:0", requires_grad=grad)   # noqa: E731
    if views:
        wide_np = np.zeros((B, Lq, 3, H, hd), np.float32)
        wide_np[:, :, 1] = q_np
        cache_np = [np.concatenate([a, np.ones((B, 11, H, hd), np.float32)], 1) for a in (k_np, v_np)]
        wide, kc, vc = tensor(wide_np), tensor(cache_np[0]), tensor(cache_np[1])
        q, k, v = wide[:, :, 1], kc[:, :Lk], vc[:, :Lk]
    else:
        q, k, v = tensor(q_np), tensor(k_np), tensor(v_np)
    node = fused.attention(q, k, v, causal=True, start_pos=start, window=W if window == "case" else window)
    (node * tensor(w_np, False)).sum().backward()
    grads = [wide.grad.get()[:, :, 1], kc.grad.get()[:, :Lk], vc.grad.get()[:, :Lk]] if views else \
        [t.grad.get() for t in (q, k, v)]
    return node._kind, [node.numpy()] + grads


def _close(got, ref, what):
    err, size = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{what}: err {err:.3e} size {size:.3e}")
    assert got.shape == ref.shape and size > 0 and err <= 1e-4 * size, (what, err, size)


@pytest.mark.parametrize("case", CASES)
def test_band_kernels_match_float64(hip, case):
    kind, got = _run(case)
    assert kind == "band"
    for what, a, b in zip(("o", "dq", "dk", "dv"), got, _ref(*_inputs(case), case[3], case[5])):
        if b.any():
            _close(a, b, f"{case} {what}")
        else:                                 # (W = 1: the softmax of one key has no gradient -- the bound is 0)
            assert a.shape == b.shape and not a.any(), (case, what)


def test_window_of_one_returns_v_exactly(hip):
    assert np.array_equal(_run(CASES[2])[1][0], _inputs(CASES[2])[2])


def test_window_past_the_sequence_is_causal_attention(hip):
    kind, plain = _run(CASES[3], None)
    assert kind != "band"
    for what, a, b in zip(("o", "dq", "dk", "dv"), _run(CASES[3])[1], plain):
        _close(a, b, f"W >= L against window=None, {what}")


def test_keys_no_query_sees_get_exact_zeros(hip):
    _, (o, dq, dk, dv) = _run(CASES[4])
    assert not dk[:, :45].any() and not dv[:, :45].any() and dk[:, 45:].all() and dv[:, 45:].all()


def test_band_backward_is_deterministic(hip):
    first, second = _run(CASES[0])[1], _run.__wrapped__(CASES[0])[1]
    assert all(np.array_equal(a, b) and np.isfinite(a).all() for a, b in zip(first, second))


def test_band_header_and_exports_agree():
    from pydynet_amd import _lib
    protos = _lib.parse_header(_lib.BAND_HEADER_PATHS[0])
    assert len(protos) == 4 and all(n.startswith("pdnb_") for n in protos) and not set(protos) & set(_lib.parse_header())
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnb_")}
    assert exported == set(protos), exported ^ set(protos)
