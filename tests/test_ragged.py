"""Ragged-batch generation (`Llama.generate_ragged`: prompts of different lengths, a position per row, stop ids) on the
CPU: the `cpu` device (the NumPy statement, `Attention.step_rows`) and the emulated C ABI with the per-row entry points
of tests/abi_emulator/_decode_rows.py (the graph-path plan, the three- and two-launch layers, the generic HIP step)."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters

V = 64


def _model(dev, B=5, D=96, H=2, seq=32, seed=5):
    """head_dim 48 (D = 96, H = 2): the two-launch layer; H = 4: head_dim 24, the three-launch layer."""
    np.random.seed(seed)
    m = Llama(V, D, H, 96, seq, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(V, D).astype(np.float32)
    m.lm_head.weight.data[...] *= 8.0                  # logits of a few units: clear argmax margins, draws off the argmax
    return m.to(dev) if dev != "cpu" else m


def _run(it):
    try:
        with pdn.no_grad():
            return [t.numpy().reshape(-1).copy() for t in it]
    finally:
        pdn.autograd.set_grad_enabled(True)


def _ragged(m, prompts, n, **kw):
    m.eval()
    try:
        return np.stack(_run(m.generate_ragged(prompts, n, **kw)), 1) if n else np.zeros((len(prompts), 0), np.int64)
    finally:
        m.train(True)


def _gen(m, prompt, total, **kw):
    m.eval()
    try:
        return np.stack(_run(m.generate(np.asarray(prompt), total, **kw)), 1)
    finally:
        m.train(True)


def _prompts(lens, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, V, n) for n in lens]


SAMPLED = [dict(temperature=1.0, seed=3), dict(temperature=0.8, top_p=0.9, seed=11),
           dict(temperature=1.3, top_k=5, top_p=0.95, seed=2 ** 64 - 1)]


@pytest.mark.parametrize("kw", [{}] + SAMPLED)
def test_equal_lengths_match_generate_on_cpu(kw):
    ids = np.stack(_prompts([4, 4, 4], seed=1))
    ref = _gen(_model("cpu"), ids, 4 + 9, **kw)
    got = _ragged(_model("cpu"), list(ids), 9, **kw)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("kw", [{}] + SAMPLED)
def test_equal_lengths_match_generate_emulated(emulated_hip, H, kw):
    Graph.clear()
    ids = np.stack(_prompts([5, 5], seed=2))
    ref = _gen(_model("hip:0", H=H), ids, 5 + 8, **kw)
    counters()
    got = _ragged(_model("hip:0", H=H), list(ids), 8, **kw)
    c = counters()
    assert np.array_equal(got, ref)
    assert c[29] > 0                                      # the per-row entries ran
    assert np.array_equal(got, _ragged(_model("cpu", H=H), list(ids), 8, **kw))


def _margins(m, prompt, total):
    """Top-2 logit gaps of every step of `generate` on the `cpu` device (lm_head outputs recorded on the way)."""
    seen = []
    fwd = m.lm_head.forward

    def rec(x):
        y = fwd(x)
        seen.append(np.asarray(y.numpy())[:, -1, :])
        return y
    m.lm_head.forward = rec
    try:
        toks = _gen(m, prompt, total)
    finally:
        del m.lm_head.forward
    s = np.sort(np.concatenate(seen), -1)
    return toks, s[:, -1] - s[:, -2]


@pytest.mark.parametrize("B", [1, 2, 3, 5])
def test_ragged_rows_match_single_prompt_generate(B):
    lens = [1, 7, 3, 5, 2][:B]
    prompts = _prompts(lens, seed=B)
    n = 9
    got = _ragged(_model("cpu"), prompts, n)
    for b, p in enumerate(prompts):
        toks, gap = _margins(_model("cpu"), p[None], len(p) + n)
        assert len(gap) == n and gap.min() > 1e-3        # no near-tie anywhere: the comparison is not luck
        assert np.array_equal(got[b], toks[0]), b


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("kw", [{}] + SAMPLED[1:])
def test_ragged_emulated_equals_cpu(emulated_hip, H, kw):
    Graph.clear()
    prompts = _prompts([1, 6, 3, 8, 2], seed=7)
    cpu = _ragged(_model("cpu", H=H), prompts, 10, **kw)
    counters()
    emu = _ragged(_model("hip:0", H=H), prompts, 10, **kw)
    assert counters()[29] > 0
    assert np.array_equal(emu, cpu)


@pytest.mark.parametrize("kw", [{}, SAMPLED[0]])
def test_ragged_generic_step_beyond_the_plan(emulated_hip, kw):
    """B = 12 > 8 and the wide step off: the generic HIP step with pdn_attention_decode_rows_f32."""
    Graph.clear()
    prompts = _prompts([1 + i % 6 for i in range(12)], seed=12)
    cpu = _ragged(_model("cpu", B=12), prompts, 7, **kw)
    Llama.wide_decode = False
    try:
        counters()
        emu = _ragged(_model("hip:0", B=12), prompts, 7, **kw)
        assert counters()[29] > 0
    finally:
        Llama.wide_decode = True
    assert np.array_equal(emu, cpu)


@pytest.mark.parametrize("fast", [True, False])
def test_unfused_and_module_paths_on_emulated(emulated_hip, fast):
    Graph.clear()
    prompts = _prompts([2, 5, 1], seed=4)
    cpu = _ragged(_model("cpu"), prompts, 8)
    Llama.fast_decode, Llama.fused_decode = fast, 0
    try:
        assert np.array_equal(_ragged(_model("hip:0"), prompts, 8), cpu)
    finally:
        Llama.fast_decode, Llama.fused_decode = True, 2


def _first_hit(row, stop):
    hits = [i for i, t in enumerate(row) if t in stop]
    return hits[0] if hits else len(row) - 1


@pytest.mark.parametrize("dev", ["cpu", "hip:0"])
def test_stop_ids(emulated_hip, dev):
    Graph.clear()
    prompts = _prompts([3, 6, 2], seed=9)
    free = _ragged(_model("cpu"), prompts, 12)
    stop = {int(free[0, 2]), int(free[2, 5])}          # row 0 stops by its 3rd token, row 2 by its 6th
    m = _model(dev)
    before = [np.array(l.attention.cache_k.numpy()) for l in m.layers]
    got = _ragged(m, prompts, 12, stop_ids=stop)
    ends = [_first_hit(free[b], stop) for b in range(3)]
    assert got.shape[1] == max(ends) + 1                  # the iterator ends at the step where the last row stopped
    for b in range(3):
        end = ends[b]
        assert np.array_equal(got[b, :end + 1], free[b, :end + 1])
        assert (got[b, end + 1:] == -1).all()
        # its position stopped advancing: no cache slot beyond its last decode step was written
        last = len(prompts[b]) + end
        for l, k0 in zip(m.layers, before):
            assert np.array_equal(l.attention.cache_k.numpy()[b, last + 1:], k0[b, last + 1:])


def test_all_rows_stopped_by_the_prompt_pass_yields_one_step(emulated_hip):
    prompts = _prompts([3, 4], seed=3)
    first = _ragged(_model("hip:0", B=2), prompts, 1)[:, 0]
    got = _ragged(_model("hip:0", B=2), prompts, 10, stop_ids=set(first.tolist()))
    assert got.shape == (2, 1) and np.array_equal(got[:, 0], first)


@pytest.mark.parametrize("bad", [
    dict(prompts=[[1, 2], []]),                                   # an empty prompt
    dict(prompts=[[1]] * 6),                                      # B > max_batch_size
    dict(prompts=[[1, 64]]),                                      # an id outside [0, vocab)
    dict(prompts=[[1, -1]]),
    dict(prompts=[[1, 2]], stop_ids=[64]),                        # a stop id outside [0, vocab)
    dict(prompts=[[1] * 20, [2]], n=13),                          # a row whose last position is 32 >= max_seq_len
    dict(prompts=[[1, 2]], temperature=-1.0),                     # sampling arguments (check_sampling_args)
    dict(prompts=[[1, 2]], top_p=0.0),
    dict(prompts=[[1, 2]], n=-1),
    dict(prompts=[]),
])
def test_invalid_arguments_raise_before_anything_runs(emulated_hip, bad):
    m = _model("hip:0")
    counters()
    kw = dict(bad)
    prompts, n = kw.pop("prompts"), kw.pop("n", 4)
    with pytest.raises(ValueError):
        m.generate_ragged(prompts, n, **kw)                       # (not iterated: the call itself refuses)
    assert not any(counters())
    assert getattr(m, "_decode_st", None) is None


def test_last_position_bound_is_per_row(emulated_hip):
    m = _model("hip:0", B=2)
    assert _ragged(m, [[1] * 20, [2]], 12).shape == (2, 12)       # row 0's last step at position 31: accepted


def test_ragged_then_rectangular_then_ragged(emulated_hip):
    """One model, three generations: the tokens are those of the same sequence on the `cpu` device (`generate` reads
    cache slot L, which no step writes -- as the reference's -- so each run depends on the ones before it), and the
    rectangular run re-plans exactly as `generate` alone does: same key, graphs, launches, slot 29 at zero."""
    Graph.clear()
    prompts = _prompts([2, 6, 4], seed=5)
    ids = np.stack(_prompts([4, 4, 4], seed=6))
    fresh = _model("hip:0")
    counters()
    _gen(fresh, ids, 14)
    c_rect = counters()
    key_ref = fresh._decode_st["key"]
    cpu = _model("cpu")
    ref = [_ragged(cpu, prompts, 9), _gen(cpu, ids, 14), _ragged(cpu, prompts, 9)]
    m = _model("hip:0")
    assert np.array_equal(_ragged(m, prompts, 9), ref[0])
    counters()
    assert np.array_equal(_gen(m, ids, 14), ref[1])
    c = counters()
    assert c == c_rect and c[29] == 0
    st = m._decode_st
    assert st["key"][:5] + st["key"][6:] == key_ref[:5] + key_ref[6:]      # (element 5: the weights' addresses)
    assert not st["ragged"] and set(st["graphs"]) == set(fresh._decode_st["graphs"])
    assert np.array_equal(_ragged(m, prompts, 9), ref[2])
    assert m._decode_st["ragged"]
