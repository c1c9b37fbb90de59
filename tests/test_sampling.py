"""Sampled generation (pydynet_amd/llm/sampling.py, csrc/sample.hip) on the CPU: the Philox generator against NumPy's own,
properties of the NumPy statement of the contract, and `Llama.generate(..., temperature=...)` on the `cpu` device and on
the emulated C ABI (tests/abi_emulator/_sampling.py), greedy mode unchanged."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters


def word0(counter, key):
    return int(sampling.philox4x64(np.array(counter, np.uint64), np.array(key, np.uint64))[0])


def test_philox_known_answers():
    assert word0([0, 0, 0, 0], [0, 0]) == 0x16554d9eca36314c
    assert word0([1, 0, 0, 0], [0, 0]) == 0x02f4ba6408e4d89b
    assert word0([6, 3, 0, 0], [1234, 0]) == 0x65c8dfd4ce6f922c
    assert np.random.Philox(counter=[0, 0, 0, 0], key=[0, 0]).random_raw() == 0x02f4ba6408e4d89b
    assert np.random.Philox(counter=[5, 3, 0, 0], key=[1234, 0]).random_raw() == 0x65c8dfd4ce6f922c


def test_philox_matches_numpy():
    """np.random.Philox adds 1 to its counter before the first block, and its first raw word is the block's first word."""
    rng = np.random.default_rng(7)
    ctr = rng.integers(0, 2 ** 63, (300, 4), dtype=np.uint64)
    ctr[:100, 1:] = 0                                       # the (t, b, 0, 0) shape the sampler uses
    key = rng.integers(0, 2 ** 63, (300, 2), dtype=np.uint64)
    ours = sampling.philox4x64(ctr + np.array([1, 0, 0, 0], np.uint64), key)
    for i in range(300):
        g = np.random.Philox(counter=[int(v) for v in ctr[i]], key=[int(v) for v in key[i]])
        assert [g.random_raw() for _ in range(4)] == [int(v) for v in ours[i]], i


def test_uniforms_are_24_bit_and_in_range():
    u = sampling.uniforms(5, np.arange(4096), 99)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)         # exact in fp32


def test_top_k_one_and_tiny_top_p_are_the_argmax():
    z = np.random.default_rng(0).standard_normal((50, 300)) * 3
    for seed in range(3):
        assert np.array_equal(sampling.sample_rows_np(z, 11, 0.7, 1, 1.0, seed), z.argmax(-1))
        assert np.array_equal(sampling.sample_rows_np(z, 11, 2.5, 0, 1e-9, seed), z.argmax(-1))


def test_ties_at_the_thresholds_are_all_kept():
    # top-k: the 2nd largest value appears three times -> k = 2 keeps all four top tokens
    z = np.array([[0.0, 3.0, 1.0, 1.0, -2.0, 1.0]])
    got = {int(sampling.sample_rows_np(z, t, 5.0, 2, 1.0, 1)[0]) for t in range(400)}
    assert got == {1, 2, 3, 5}
    # top-p: two equal top logits, a tiny top_p keeps both
    z = np.array([[2.0, 0.5, 2.0, -1.0]])
    got = {int(sampling.sample_rows_np(z, t, 1.0, 0, 1e-6, 1)[0]) for t in range(400)}
    assert got == {0, 2}
    # mass of {z >= theta} exactly reaching top_p: theta is that value (the next one is not kept)
    z = np.log(np.array([[0.5, 0.25, 0.25]]))
    got = {int(sampling.sample_rows_np(z, t, 1.0, 0, 0.5, 3)[0]) for t in range(200)}
    assert got == {0}


def test_distribution_follows_the_contract():
    z = np.array([1.0, 0.0, 2.0, -1.0, 0.5])
    T, n = 0.9, 20000
    ids = sampling.sample_rows_np(np.broadcast_to(z, (n, 5)), 3, T, 0, 1.0, 5)
    p = np.exp(z / T) / np.exp(z / T).sum()
    freq = np.bincount(ids, minlength=5) / n
    assert np.abs(freq - p).max() < 0.015


def test_result_is_independent_of_row_order():
    z = np.random.default_rng(1).standard_normal((17, 90))
    ref = sampling.sample_rows_np(z, 4, 1.1, 20, 0.8, 77)
    perm = np.random.default_rng(2).permutation(17)
    assert np.array_equal(sampling.sample_rows_np(z[perm], 4, 1.1, 20, 0.8, 77, rows=perm), ref[perm])


def _tiny(dev, B=2, seed=5):
    np.random.seed(seed)
    m = Llama(64, 48, 2, 96, 32, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(64, 48).astype(np.float32)
    m.lm_head.weight.data[...] *= 8.0                  # logits of a few units: draws that differ from the argmax
    return m.to(dev) if dev != "cpu" else m


def _gen(m, prompt, total, **kw):
    m.eval()                                               # (also turns gradients off, model.py-style: restored below)
    try:
        with pdn.no_grad():
            return np.concatenate([t.numpy() for t in m.generate(prompt, total, **kw)], axis=1)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


PROMPT = np.array([[1, 5, 9, 2], [7, 7, 3, 0]])


@pytest.mark.parametrize("bad", [dict(temperature=-0.1), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
                                 dict(seed=-1), dict(seed=2 ** 64), dict(top_k=1.5)])
def test_invalid_arguments_raise_before_anything_runs(bad):
    m = _tiny("cpu")
    with pytest.raises(ValueError):
        m.generate(PROMPT, 10, **bad)                     # (not iterated: the call itself refuses)


def test_default_generate_is_greedy_with_unchanged_launches(emulated_hip):
    Graph.clear()
    m = _tiny("hip:0")
    counters()
    base = _gen(m, PROMPT, 14)
    c0 = counters()
    again = _gen(_tiny("hip:0"), PROMPT, 14, temperature=0.0, top_k=3, top_p=0.5, seed=9)   # ignored at T = 0
    c1 = counters()
    assert np.array_equal(base, again) and c0 == c1 and c0[28] == 0
    # the module path's argmax
    Llama.fast_decode = False
    try:
        assert np.array_equal(_gen(_tiny("hip:0"), PROMPT, 14), base)
    finally:
        Llama.fast_decode = True


@pytest.mark.parametrize("kw", [dict(temperature=1.0, seed=3), dict(temperature=0.8, top_p=0.9, seed=11),
                                dict(temperature=1.3, top_k=5, top_p=0.95, seed=2 ** 64 - 1)])
def test_sampled_generate_emulated_equals_cpu(emulated_hip, kw):
    Graph.clear()
    cpu = _gen(_tiny("cpu"), PROMPT, 16, **kw)
    counters()
    emu = _gen(_tiny("hip:0"), PROMPT, 16, **kw)
    assert counters()[28] == 16 - PROMPT.shape[1]          # one sample launch per generated position
    assert np.array_equal(emu, cpu)
    assert not np.array_equal(cpu, _gen(_tiny("cpu"), PROMPT, 16))       # (the draws do leave the argmax)
    assert np.array_equal(cpu, _gen(_tiny("cpu"), PROMPT, 16, **kw))     # reproducible


@pytest.mark.parametrize("dev", ["cpu", "hip:0"])
def test_top_k_one_gives_the_greedy_tokens(emulated_hip, dev):
    greedy = _gen(_tiny(dev), PROMPT, 14)
    for T in (0.3, 1.0, 4.0):
        assert np.array_equal(_gen(_tiny(dev), PROMPT, 14, temperature=T, top_k=1, seed=int(T * 10)), greedy)


@pytest.mark.parametrize("fast", [True, False])
def test_sampled_then_greedy_on_one_model(emulated_hip, fast):
    Llama.fast_decode = fast
    try:
        greedy = _gen(_tiny("hip:0"), PROMPT, 14)
        m = _tiny("hip:0")
        first = _gen(m, PROMPT, 14, temperature=1.0, seed=4)
        assert np.array_equal(_gen(m, PROMPT, 14), greedy)
        assert np.array_equal(_gen(m, PROMPT, 14, temperature=1.0, seed=4), first)
        assert np.array_equal(_gen(m, PROMPT, 14), greedy)
    finally:
        Llama.fast_decode = True


def test_generic_step_samples_beyond_the_plan(emulated_hip):
    """B > 8 and the wide step off: the decode step of the library's generic entry points ends in pdn_sample_rows_f32."""
    Graph.clear()
    prompt = np.random.default_rng(3).integers(0, 64, (9, 3))
    kw = dict(temperature=0.9, top_p=0.9, seed=21)
    Llama.wide_decode = False
    try:
        got = _gen(_tiny("hip:0", B=9), prompt, 10, **kw)
    finally:
        Llama.wide_decode = True
    assert np.array_equal(got, _gen(_tiny("cpu", B=9), prompt, 10, **kw))
