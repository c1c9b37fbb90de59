"""Beam search on a real MI355X: pdn_beam_topk_rows_f32 against float64 NumPy, pdn_kv_reorder_rows_f32 against a NumPy
gather, determinism, and `Llama.beam_search` end to end on every path against the `cpu` device."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters

pytestmark = pytest.mark.gpu
f32 = np.float32


def _topk(hip, z, W, stops, pos=None):
    B, V = z.shape
    S = len(stops)
    Z = hip.from_numpy(z)
    cl, ci, sl = hip.zeros((B, W), f32), hip.zeros((B, W), np.int32), hip.zeros((B, max(S, 1)), f32)
    st = hip.from_numpy(np.array(list(stops) or [0], np.int32))
    P = hip.from_numpy(np.asarray(pos, np.int32)) if pos is not None else None
    _lib.lib().call("pdn_beam_topk_rows_f32", Z._ptr, V, B, V, W, 0, P._ptr if P is not None else None, st._ptr, S,
                    cl._ptr, ci._ptr, sl._ptr, hip.stream())
    return cl.get(), ci.get(), sl.get()[:, :S]


@pytest.mark.parametrize("V, B", [(64, 256), (32000, 40), (50257, 9)])
@pytest.mark.parametrize("W", [1, 4, 16])
def test_topk_against_float64(hip, V, B, W):
    rng = np.random.default_rng(V + W)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    z[:, 5:9] = z[:, [3]]                                     # ties at the top: ids 3, 5 .. 8 share the row maximum
    z[:, 3] += 8
    z[:, 5:9] += 8
    stops = (6, V - 1, 0)
    pos = np.where(np.arange(B) % 7 == 3, -1, 5)
    counters()
    lp, ids, slp = _topk(hip, z, W, stops, pos)
    assert counters()[32] == 1
    z64 = z.astype(np.float64)
    lse = z64.max(1) + np.log(np.exp(z64 - z64.max(1, keepdims=True)).sum(1))
    for r in np.flatnonzero(pos >= 0):
        key = np.where(np.isin(np.arange(V), stops), -np.inf, z64[r])
        want = np.lexsort((np.arange(V), -key))[:W]
        assert ids[r].tolist() == want.tolist(), r
        assert np.allclose(lp[r], z64[r, want] - lse[r], rtol=0, atol=2e-6 * max(1, abs(lse[r])))
        assert np.allclose(slp[r], z64[r, list(stops)] - lse[r], rtol=0, atol=2e-6 * max(1, abs(lse[r])))


def test_topk_is_deterministic(hip):
    z = (3 * np.random.default_rng(1).standard_normal((64, 32000))).astype(f32)
    a, b = _topk(hip, z, 8, (1, 2)), _topk(hip, z, 8, (1, 2))
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("case", ["swap", "cycle", "fanout", "stopped"])
def test_reorder_against_gather(hip, case):
    B, T, D, n_t = 24, 40, 288, 3
    rng = np.random.default_rng(len(case))
    caches = [rng.standard_normal((B, T, D)).astype(f32) for _ in range(n_t)]
    parent = np.arange(B)
    pos = rng.integers(1, T + 1, B)
    if case == "swap":
        parent[[2, 7]] = parent[[7, 2]]
        pos[[2, 7]] = 17
    elif case == "cycle":
        parent[4:12] = np.roll(np.arange(4, 12), 1)
        pos[4:12] = T
    elif case == "fanout":
        parent[8:16] = 8
        pos[8:16] = 21
    else:
        parent = rng.permutation(B)
        pos[::3] = -1
    dev = [hip.from_numpy(c) for c in caches]
    ptrs = hip.from_numpy(np.array([d._ptr for d in dev], np.int64))
    P, Q = hip.from_numpy(parent.astype(np.int32)), hip.from_numpy(pos.astype(np.int32))
    counters()
    _lib.lib().call("pdn_kv_reorder_rows_f32", ptrs._ptr, n_t, T * D, B, T, D, P._ptr, Q._ptr, hip.stream())
    assert counters()[32] == 1
    for c, d in zip(caches, dev):
        want = c.copy()
        for r in range(B):
            if parent[r] != r and pos[r] > 0:
                want[r, :pos[r]] = c[parent[r], :pos[r]]
        assert np.array_equal(d.get(), want)


def _model(dev, B):
    np.random.seed(11)
    m = Llama(32000, 288, 6, 768, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(32000, 288).astype(np.float32)
    m.lm_head.weight.data[...] *= 4.0
    return m.to(dev) if dev != "cpu" else m


def _run(m, prompts, n, W, stops):
    m.eval()
    try:
        with pdn.no_grad():
            return m.beam_search(prompts, n, W, length_penalty=1.0, stop_ids=stops)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _check(got, ref):
    """Equal hypotheses; where one differs, the reference's float64 gap between it and the one the GPU took must be a
    near-tie (below 1e-4 * max(1, |score|)) -- fp32 sums in another order decide such ties either way."""
    for g, (a, b) in enumerate(zip(got, ref)):
        assert len(a) == len(b)
        for (ta, sa), (tb, sb) in zip(a, b):
            tol = 1e-4 * max(1.0, abs(sb))
            if np.array_equal(ta, tb):
                assert abs(sa - sb) <= tol, (g, sa, sb)
                continue
            other = [s for t, s in b if np.array_equal(t, ta)]
            assert abs(sa - sb) <= tol and (not other or abs(other[0] - sb) <= tol), (g, ta, sa, tb, sb)


PROMPTS = [[5, 900, 31000], [7], [2, 3, 4, 5, 6, 100], [44, 45]]


@pytest.mark.parametrize("mode", ["fused2", "fused1", "unfused", "nograph", "generic", "wide", "module"])
def test_beam_search_paths_against_cpu(hip, mode):
    Graph.clear()
    W = 4 if mode in ("wide", "generic") else 2
    B = len(PROMPTS) * W
    stops = (17, 200, 31999)
    ref = _run(_model("cpu", B), PROMPTS, 8, W, stops)
    Llama.fused_decode = {"fused2": 2, "fused1": 1}.get(mode, 0 if mode == "unfused" else 2)
    Llama.graph_decode = mode != "nograph"
    Llama.fast_decode = mode != "module"
    Llama.wide_decode = mode != "generic"
    try:
        m = _model("hip:0", B)
        counters()
        got = _run(m, PROMPTS, 8, W, stops)
        c = counters()
        _check(got, ref)
        if mode != "module":
            assert c[32] >= 3
        if mode == "wide":
            assert m._decode_st["wide"] and m._decode_st["beam"] == W
        again = _run(m, PROMPTS, 8, W, stops)                  # determinism: the same bits twice
        assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] for ga, gb in zip(got, again) for x, y in zip(ga, gb))
    finally:
        Llama.fused_decode, Llama.graph_decode, Llama.fast_decode, Llama.wide_decode = 2, True, True, True


def test_launch_count(hip):
    """Slot 32: three launches for the prompt pass and three per decode step (no group ends: no stop ids)."""
    Graph.clear()
    Llama.graph_decode = False                                   # (a graph replay calls no entry point: nothing counted)
    try:
        m = _model("hip:0", 8)
        counters()
        _run(m, PROMPTS[:2], 6, 4, ())
        assert counters()[32] == 3 * 6
    finally:
        Llama.graph_decode = True
