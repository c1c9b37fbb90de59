"""Prefix caching on a real MI355X: pdn_kv_copy_prefix_rows_f32 (csrc/prefix.hip) bit-exact against the NumPy statement of
tests/abi_emulator/_extend.py, and `Llama.serve(prefill_chunk=C, prefix_cache=k)` end to end against the `cpu`
generate_ragged reference under the first-difference margin rule of tests/test_serve_gpu.py, with at most one request of a
case differing at all (tests/test_prefix.py: `compare`; its `test_gpu_reference_alone_shows_no_difference` checks on the
CPU that the reference run of these requests has no near-tie of its own)."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from tests.abi_emulator import copy_prefix_np, counters
from tests.test_prefix import CASES, GPU_SEED, PEN, _k, compare, requests, simulate
from tests.test_serve_gpu import SAMPLED, _model, _ragged_reference, _serve_all

pytestmark = pytest.mark.gpu
f32 = np.float32

# (dst, src, len) over 10 rows of 40 positions: a swap, a 3-chain (one link the cache's length, one past it: clamped), one
# source feeding three rows (lengths 1, 13 and 0: skipped), a row onto itself and rows outside the cache (skipped)
COPIES = [(0, 1, 7), (1, 0, 12), (2, 3, 40), (3, 4, 55), (6, 5, 1), (7, 5, 13), (8, 5, 0), (9, 9, 5), (9, 12, 5), (-1, 0, 5),
          (10, 0, 5), (4, -2, 3)]


def _caches(hip, n_t, n_rows, max_len, pad, D):
    """n_t caches of (n_rows, max_len + pad, D) distinct floats (exact in fp32), so that a stray write shows."""
    host = [(j * n_rows * (max_len + pad) * D + np.arange(n_rows * (max_len + pad) * D)).astype(f32).reshape(
        n_rows, max_len + pad, D) for j in range(n_t)]
    assert host[-1].max() < 2 ** 24
    dev = [hip.from_numpy(a) for a in host]
    return host, dev, hip.from_numpy(np.array([a._ptr for a in dev], np.int64))


def _launch(hip, tab, n_t, n_rows, max_len, pad, D, copies):
    d, s, n = (hip.from_numpy(np.array([c[i] for c in copies] or [0], np.int32)) for i in range(3))
    _lib.lib().call("pdn_kv_copy_prefix_rows_f32", tab._ptr, n_t, (max_len + pad) * D, n_rows, max_len, D, d._ptr, s._ptr,
                    n._ptr, len(copies), hip.stream())


@pytest.mark.parametrize("pad", [0, 3])                           # 3: a row stride past the positions the entry may touch
@pytest.mark.parametrize("n_t", [12, 2])
@pytest.mark.parametrize("D", [96, 288, 30])                      # 30: not a multiple of 4 (the scalar path)
def test_kv_copy_prefix_rows(hip, D, n_t, pad):
    n_rows, max_len = 10, 40
    host, dev, tab = _caches(hip, n_t, n_rows, max_len, pad, D)
    counters()
    _launch(hip, tab, n_t, n_rows, max_len, pad, D, [])           # no copies: nothing launched, nothing written
    assert counters()[38] == 0
    assert all(np.array_equal(a.get(), h) for a, h in zip(dev, host))
    _launch(hip, tab, n_t, n_rows, max_len, pad, D, COPIES)
    assert counters()[38] == 1
    want = [h.copy() for h in host]
    copy_prefix_np([w[:, :max_len] for w in want], *zip(*COPIES))
    got = [a.get() for a in dev]
    for j in range(n_t):
        assert np.array_equal(got[j], want[j]), j                 # bit-exact; every float outside the copies unchanged
    assert not np.array_equal(got[0][0, :7], host[0][0, :7]) and np.array_equal(got[0][0, :7], host[0][1, :7])
    assert np.array_equal(got[0][1, :12], host[0][0, :12])        # the swap: both rows as they were before the launch
    assert np.array_equal(got[0][2], host[0][3]) if pad == 0 else np.array_equal(got[0][2, :40], host[0][3, :40])
    assert np.array_equal(got[0][3, :40], host[0][4, :40])        # the chain: row 3 gives its old contents, takes row 4's
    # the same launch from the same start: the same bits
    _, dev2, tab2 = _caches(hip, n_t, n_rows, max_len, pad, D)
    _launch(hip, tab2, n_t, n_rows, max_len, pad, D, COPIES)
    assert all(np.array_equal(a.get(), g) for a, g in zip(dev2, got))


@pytest.mark.parametrize("D,n", [(96, 40), (30, 40), (96, 256), (30, 200)])   # 40: 6 positions per group; 256: one
def test_kv_copy_prefix_rows_many_copies(hip, D, n):
    """A cycle over n rows (row i takes row i + 1's, the last the first's) with a length per copy."""
    max_len, n_t = 24, 2
    host, dev, tab = _caches(hip, n_t, n, max_len, 0, D)
    lens = np.random.default_rng(n + D).integers(0, max_len + 5, n)
    copies = [(i, (i + 1) % n, int(lens[i])) for i in range(n)]
    _launch(hip, tab, n_t, n, max_len, 0, D, copies)
    want = [h.copy() for h in host]
    copy_prefix_np(want, *zip(*copies))
    assert all(np.array_equal(a.get(), w) for a, w in zip(dev, want))


def test_kv_copy_prefix_rows_refuses_bad_arguments(hip):
    host, dev, tab = _caches(hip, 1, 4, 8, 0, 16)
    L, one = _lib.lib(), hip.from_numpy(np.zeros(300, np.int32))
    for args in ((tab._ptr, 1, 8 * 16, 4, 8, 16, one._ptr, one._ptr, one._ptr, 257),     # more than 256 copies
                 (tab._ptr, 1, 8 * 16 - 1, 4, 8, 16, one._ptr, one._ptr, one._ptr, 1),   # rows that overlap
                 (tab._ptr, 1, 8 * 16, 4, 8, 16, None, one._ptr, one._ptr, 1)):
        with pytest.raises(_lib.HipLibraryError):
            L.call("pdn_kv_copy_prefix_rows_f32", *args, hip.stream())
    assert np.array_equal(dev[0].get(), host[0])


# -- end to end ----------------------------------------------------------------------------------------------------------
E2E = [(S, C, cache, kw) for S, C, cache in CASES for kw in ({}, SAMPLED)] + [(3, 4, True, PEN), (5, 64, 2, PEN)]


@pytest.mark.parametrize("S,C,cache,kw", E2E)
def test_serve_prefix_cache_end_to_end(hip, S, C, cache, kw):
    Graph.clear()
    prompts, budgets = requests(256, GPU_SEED)
    ref, logits = _ragged_reference(prompts, budgets, **kw)
    want = [ref[r, :n] for r, n in enumerate(budgets)]
    m = _model("hip:0", 8)
    counters()
    got = _serve_all(m, prompts, budgets, slots=S, prefill_chunk=C, prefix_cache=cache, **kw)
    c = counters()
    compare(got, want, logits, prompts, kw)
    st, kinds = simulate(prompts, budgets, S, C, _k(cache))
    assert m.prefix_stats == st, (m.prefix_stats, st)
    assert st["reused_tokens"] > 0 and st["copies"] > 0 and {"own", "copy"} <= kinds
    assert c[38] == st["launches"] > 0 and c[33] > 0
    assert any(len(k) > 2 and k[2] == "mixed" for k in m._decode_st["graphs"]), "no mixed step captured"
    # the same model again (its rows now hold the last run's prompts, which a new run must not trust): the same tokens
    again = _serve_all(m, prompts, budgets, slots=S, prefill_chunk=C, prefix_cache=cache, **kw)
    compare(again, want, logits, prompts, kw)
    assert m.prefix_stats == st


@pytest.mark.parametrize("S,C,cache", CASES[:2])
def test_serve_prefix_cache_logprobs(hip, S, C, cache):
    Graph.clear()
    prompts, budgets = requests(256, GPU_SEED)
    ref, logits = _ragged_reference(prompts, budgets)
    want = [ref[r, :n] for r, n in enumerate(budgets)]
    cpu = _serve_all(_model("cpu", 8), prompts, budgets, slots=S, prefill_chunk=C, logprobs=2)
    m = _model("hip:0", 8)
    got = _serve_all(m, prompts, budgets, slots=S, prefill_chunk=C, logprobs=2, prefix_cache=cache)
    same = compare([g[0] for g in got], want, logits, prompts, {})
    for (_, g), (t, w), n in zip(got, cpu, same):
        n = min(n, len(t))
        # (the tolerance of tests/test_logprobs.py between two fp32 paths: ranks exact, values within 1e-4)
        assert np.allclose(g.token[:n], w.token[:n], rtol=0, atol=1e-4)
        assert np.array_equal(g.top_ids[:n], w.top_ids[:n])
        assert np.allclose(g.top_logprobs[:n], w.top_logprobs[:n], rtol=0, atol=1e-4)
    assert m.prefix_stats["copies"] > 0


def test_everything_else_leaves_counter_38_alone(hip):
    Graph.clear()
    prompts, budgets = requests(256, GPU_SEED)
    m = _model("hip:0", 8)
    counters()
    _serve_all(m, prompts, budgets, slots=4)
    _serve_all(m, prompts, budgets, slots=4, prefill_chunk=16)
    _serve_all(m, prompts, budgets, slots=4, prefill_chunk=16, prefix_cache=False)
    m.eval()
    try:
        with pdn.no_grad():
            for kw in ({}, SAMPLED):
                for _ in m.generate(np.array([[1, 2, 3]] * 3), 20, **kw):
                    pass
                for _ in m.generate_ragged([[1, 2], [3], [4, 5, 6]], 15, stop_ids=[7], **kw):
                    pass
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
    c = counters()
    assert c[38] == 0 and c[33] > 0 and c[30] > 0
    assert not hasattr(m, "prefix_stats") and "prefix" not in m._decode_st
    _serve_all(m, prompts, budgets, slots=4, prefill_chunk=16, prefix_cache=True)
    assert counters()[38] == m.prefix_stats["launches"] > 0
