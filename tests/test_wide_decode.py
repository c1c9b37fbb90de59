"""The wide decode step (9 .. 256 rows, csrc/decode_wide.hip) on the CPU: the emulated C ABI with the entry points of
tests/abi_emulator/_decode_rows.py against the `cpu` device (the module path).  `generate`, `generate_ragged` and `serve`
past 8 rows take the wide plan and give the module path's tokens, greedy and sampled; `Llama.wide_decode = False`, more than
256 rows and shapes the wide step does not take keep the generic step."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters

V = 64
SAMPLED = dict(temperature=0.9, top_k=20, top_p=0.95, seed=7)


def _model(dev, B, D=96, H=2, F=96, seq=32, seed=5):
    np.random.seed(seed)
    m = Llama(V, D, H, F, seq, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(V, D).astype(np.float32)
    m.lm_head.weight.data[...] *= 8.0                  # logits of a few units: clear argmax margins
    return m.to(dev) if dev != "cpu" else m


def _eval(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn()
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _generate(m, ids, total, **kw):
    return _eval(m, lambda: np.concatenate([np.asarray(t.numpy()) for t in m.generate(ids, total, **kw)], 1))


def _ragged(m, prompts, n, **kw):
    return _eval(m, lambda: np.stack([np.asarray(t.numpy()).reshape(-1) for t in m.generate_ragged(prompts, n, **kw)], 1))


def _serve(m, prompts, budgets, **kw):
    return _eval(m, lambda: m.serve_all(prompts, budgets, **kw))


def _prompts(lens, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, V, n) for n in lens]


def _ids(B, L=4, seed=1):
    return np.random.default_rng(seed).integers(0, V, (B, L))


def _wide(m, B):
    st = m._decode_st
    return st["ok"] and st["wide"] and st["B"] == B


@pytest.mark.parametrize("B", [9, 16, 33])
@pytest.mark.parametrize("kw", [{}, SAMPLED])
def test_generate_on_the_wide_step(emulated_hip, B, kw):
    Graph.clear()
    ids = _ids(B)
    cpu = _generate(_model("cpu", B), ids, 12, **kw)
    m = _model("hip:0", B)
    counters()
    got = _generate(m, ids, 12, **kw)
    c = counters()
    assert np.array_equal(got, cpu)
    assert _wide(m, B) and c[31] > 0 and c[29] > 0 and (c[28] > 0) == bool(kw)


@pytest.mark.parametrize("B", [9, 16, 33])
@pytest.mark.parametrize("kw", [{}, SAMPLED])
def test_generate_ragged_with_stops_on_the_wide_step(emulated_hip, B, kw):
    Graph.clear()
    prompts = _prompts([1 + (5 * i) % 9 for i in range(B)], seed=B)
    stops = [3, 17, 40]
    cpu = _ragged(_model("cpu", B), prompts, 10, stop_ids=stops, **kw)
    m = _model("hip:0", B)
    counters()
    got = _ragged(m, prompts, 10, stop_ids=stops, **kw)
    c = counters()
    assert got.shape == cpu.shape and np.array_equal(got, cpu)
    assert _wide(m, B) and c[31] > 0 and c[29] > 0


@pytest.mark.parametrize("kw", [{}, SAMPLED])
def test_serve_on_the_wide_step(emulated_hip, kw):
    """20 requests through 12 slots, budgets from 0 to 9."""
    Graph.clear()
    prompts = _prompts([1 + (3 * i) % 8 for i in range(20)], seed=3)
    budgets = [(7 * i) % 10 for i in range(20)]
    cpu = _serve(_model("cpu", 12), prompts, budgets, stop_ids=[5], **kw)
    m = _model("hip:0", 12)
    counters()
    got = _serve(m, prompts, budgets, stop_ids=[5], **kw)
    c = counters()
    assert all(np.array_equal(g, w) for g, w in zip(got, cpu))
    assert _wide(m, 12) and m._decode_st["serve"] and c[31] > 0 and c[30] > 0


@pytest.mark.parametrize("kw", [{}, SAMPLED])
def test_wide_decode_off_keeps_the_generic_step(emulated_hip, kw):
    Graph.clear()
    B = 16
    ids, prompts = _ids(B), _prompts([2 + i % 5 for i in range(B)], seed=9)
    cpu = (_generate(_model("cpu", B), ids, 10, **kw), _ragged(_model("cpu", B), prompts, 6, **kw))
    Llama.wide_decode = False
    try:
        m, m2 = _model("hip:0", B), _model("hip:0", B)
        counters()
        got = (_generate(m, ids, 10, **kw), _ragged(m2, prompts, 6, **kw))
        c = counters()
    finally:
        Llama.wide_decode = True
    assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[1], cpu[1])
    assert c[31] == 0 and not m._decode_st["ok"] and not m2._decode_st["ok"]


def test_beyond_256_rows_takes_the_generic_step(emulated_hip):
    Graph.clear()
    B = 257
    ids = _ids(B, L=2)
    cpu = _generate(_model("cpu", B, D=32, F=32, seq=8), ids, 5)
    m = _model("hip:0", B, D=32, F=32, seq=8)
    counters()
    got = _generate(m, ids, 5)
    assert np.array_equal(got, cpu)
    assert counters()[31] == 0 and not m._decode_st["ok"]


def test_unsupported_shape_takes_the_generic_step(emulated_hip):
    """F = 90 (not a multiple of 4): pdn_decode_wide_supported refuses."""
    Graph.clear()
    B = 12
    prompts = _prompts([1 + i % 4 for i in range(B)], seed=2)
    cpu = _ragged(_model("cpu", B, F=90), prompts, 6)
    m = _model("hip:0", B, F=90)
    counters()
    got = _ragged(m, prompts, 6)
    assert np.array_equal(got, cpu)
    assert counters()[31] == 0 and not m._decode_st["ok"]


def test_at_most_8_rows_keep_their_plan(emulated_hip):
    Graph.clear()
    ids = _ids(8)
    cpu = _generate(_model("cpu", 8), ids, 10)
    m = _model("hip:0", 8)
    counters()
    got = _generate(m, ids, 10)
    assert np.array_equal(got, cpu)
    assert counters()[31] == 0 and m._decode_st["ok"] and not m._decode_st["wide"]
