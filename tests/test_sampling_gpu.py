"""Sampling kernels (csrc/sample.hip) on a real MI355X: pdn_sample_rows_f32 against the float64 NumPy statement of the
contract (pydynet_amd/llm/sampling.py), determinism, a chi-square check of the draws, and sampled `Llama.generate` on the
graph-replayed decode path against the `cpu` device.  Ids may differ only where the float64 margin between u and the
nearest decision boundary is below 1e-5 (the kernel works in fp32 / integer mass units)."""
import math

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, margin

pytestmark = pytest.mark.gpu
TIGHT = 1e-5


def launch(hip, z, t, T, k, p, seed, reps=1):
    x = hip.asarray(np.ascontiguousarray(z, np.float32))
    prm = sampling.params_buffer(T, k, p, seed)
    outs = []
    for _ in range(reps):
        out = hip.empty((z.shape[0],), np.int64)
        _lib.lib().call("pdn_sample_rows_f32", x._ptr, z.shape[1], z.shape[0], z.shape[1], prm._ptr, t, out._ptr, hip.stream())
        outs.append(out.get())
    return outs


def configs(V):
    return [(1.0, 0, 1.0), (0.7, 1, 1.0), (1.3, V, 0.9), (0.8, 50, 0.95), (2.0, 0, 0.5), (0.9, 0, 0.9)]


@pytest.mark.parametrize("V", [7, 1000, 32000, 50257])
def test_sample_rows_match_the_contract(hip, V):
    rng = np.random.default_rng(V)
    close, checked = 0, 0
    for B in (1, 3, 8, 300):
        z = (3.0 * rng.standard_normal((B, V))).astype(np.float32)
        if B == 3:
            z = np.round(z, 1)                             # many ties, at both thresholds
        for ci, (T, k, p) in enumerate(configs(V)):
            if B == 300 and ci % 2:
                continue                                   # (the float64 statement is slow for 300 wide rows)
            t, seed = 17 + ci, 1000 * ci + B
            got = launch(hip, z, t, T, k, p, seed)[0]
            want = sampling.sample_rows_np(z, t, T, k, p, seed)
            for b in np.flatnonzero(got != want):
                mg = margin(z[b], t, b, T, k, p, seed)
                assert mg < TIGHT, (V, B, (T, k, p), int(b), int(got[b]), int(want[b]), mg)
                close += 1
            checked += B
    assert close <= 3, (close, checked)


def test_two_launches_are_bit_identical(hip):
    z = (2.0 * np.random.default_rng(0).standard_normal((300, 32000))).astype(np.float32)
    for T, k, p in ((1.0, 0, 0.9), (0.8, 40, 1.0), (1.5, 0, 1.0)):
        a, b = launch(hip, z, 5, T, k, p, 7, reps=2)
        assert np.array_equal(a, b)


def test_chi_square_of_the_draws(hip):
    V, n = 24, 65536
    z = np.linspace(-2.0, 2.0, V)[::-1] + 0.3 * np.sin(np.arange(V))
    T, k, p = 0.9, 20, 0.97
    got = launch(hip, np.broadcast_to(z.astype(np.float32), (n, V)), 3, T, k, p, 12345)[0]
    _, prob = sampling.kept_mask(z.astype(np.float32).astype(np.float64), k, p, T)
    assert set(np.unique(got)) <= set(np.flatnonzero(prob > 0))
    idx = np.flatnonzero(prob > 0)
    obs, exp = np.bincount(got, minlength=V)[idx], n * prob[idx]
    chi2, dof = float(((obs - exp) ** 2 / exp).sum()), idx.size - 1
    limit = dof * (1 - 2 / (9 * dof) + 4.0 * math.sqrt(2 / (9 * dof))) ** 3     # Wilson-Hilferty, z = 4
    assert chi2 < limit, (chi2, limit, dof)


def _model(dev, B):
    np.random.seed(8)
    m = Llama(256, 96, 2, 128, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(256, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to(dev) if dev != "cpu" else m


def _gen(m, prompt, total, **kw):
    m.eval()                                               # (also turns gradients off, model.py-style: restored below)
    try:
        with pdn.no_grad():
            return np.concatenate([t.numpy() for t in m.generate(prompt, total, **kw)], axis=1)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("mode", ["fused2", "fused1", "unfused", "nograph"])
def test_sampled_generate_on_the_graph_path(hip, B, mode):
    Graph.clear()
    prompt = np.random.default_rng(B).integers(0, 256, (B, 5))
    total, kw = 40, dict(temperature=0.9, top_k=0, top_p=0.92, seed=31 + B)
    want = _gen(_model("cpu", B), prompt, total, **kw)
    Llama.fused_decode = {"fused2": 2, "fused1": 1}.get(mode, 0 if mode == "unfused" else 2)
    Llama.graph_decode = mode != "nograph"
    try:
        m = _model("hip:0", B)
        got = _gen(m, prompt, total, **kw)
        if Llama.graph_decode and B == 1:
            assert m._decode_st["graphs"] and all(key[1] for key in m._decode_st["graphs"]), "no sampled graph captured"
        assert np.array_equal(_gen(m, prompt, total, **kw), got)          # reproducible on the same model
    finally:
        Llama.fused_decode, Llama.graph_decode = 2, True
    bad = np.flatnonzero((got != want).any(0))
    if bad.size:
        s = int(bad[0])                                    # first differing step: its margin must be tiny
        seq = np.concatenate([prompt, want[:, :s]], axis=1)
        cpu = _model("cpu", B)
        with pdn.no_grad():
            lg = cpu.forward_logits(pdn.Tensor(seq, dtype=np.int64), 0).numpy()[:, -1, :]
        mg = min(margin(lg[b], prompt.shape[1] + s, b, kw["temperature"], kw["top_k"], kw["top_p"], kw["seed"])
                 for b in range(B))
        assert mg < TIGHT, (mode, B, s, mg)


def test_slot_28_counts_sampled_tokens(hip):
    Graph.clear()
    prompt = np.array([[3, 1, 4, 1, 5]])
    Llama.graph_decode = False
    try:
        m = _model("hip:0", 1)
        counters()
        _gen(m, prompt, 20, temperature=1.0, seed=2)
        assert counters()[28] == 15                        # the prompt pass + one sample tick per decode step
        _gen(m, prompt, 20)
        assert counters()[28] == 0
    finally:
        Llama.graph_decode = True
    m = _model("hip:0", 1)
    _gen(m, prompt, 20)
    assert counters()[28] == 0                             # greedy graph path: never


def test_greedy_after_sampled_uses_its_own_graph(hip):
    Graph.clear()
    prompt = np.array([[9, 8, 7]])
    greedy = _gen(_model("hip:0", 1), prompt, 30)
    m = _model("hip:0", 1)
    s1 = _gen(m, prompt, 30, temperature=1.0, seed=5)
    assert np.array_equal(_gen(m, prompt, 30), greedy)
    assert np.array_equal(_gen(m, prompt, 30, temperature=1.0, seed=5), s1)
    assert not np.array_equal(s1, greedy)
