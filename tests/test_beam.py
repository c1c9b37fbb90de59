"""Beam search (`Llama.beam_search`) on the CPU: the statement of pydynet_amd/llm/beam.py, its identities (one beam is
`generate_ragged`; enough beams give the exact top-W of all sequences), and the emulated C ABI with the entry points of
tests/abi_emulator/_beam.py (the beam plan at every fused level, rows form and wide step, graph and no graph, the
generic HIP step) against the `cpu` device, bit for bit."""
import itertools

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import beam
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters

V = 64


def _model(dev, B=8, D=96, H=2, seq=32, seed=5, vocab=V):
    np.random.seed(seed)
    m = Llama(vocab, D, H, 96, seq, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(vocab, D).astype(np.float32)
    m.lm_head.weight.data[...] *= 4.0
    return m.to(dev) if dev != "cpu" else m


def _eval(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn()
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _beam(m, prompts, n, W, **kw):
    return _eval(m, lambda: m.beam_search(prompts, n, W, **kw))


def _prompts(lens, seed=0, vocab=V):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, vocab, k) for k in lens]


def _same(a, b):
    """Equal tokens; scores to float32 rounding (the emulated decode kernels sum the logits in their own order)."""
    assert len(a) == len(b)
    for ga, gb in zip(a, b):
        assert len(ga) == len(gb)
        for (ta, sa), (tb, sb) in zip(ga, gb):
            assert np.array_equal(ta, tb) and abs(sa - sb) <= 1e-5 * max(1.0, abs(sb)), (ta, sa, tb, sb)


# -- the statement ----------------------------------------------------------------------------------------------------
def test_topk_rows_orders_by_logp_then_id_and_skips_stops():
    z = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, -1.0]], np.float32)
    lp, ids, slp = beam.topk_rows(z, 3, np.array([2]))
    assert ids.tolist() == [[1, 4, 3]]
    ref = z.astype(np.float64) - np.log(np.exp(z.astype(np.float64)).sum())
    assert np.array_equal(lp[0], ref[0, [1, 4, 3]].astype(np.float32))
    assert np.array_equal(slp[0], ref[0, [2]].astype(np.float32))


def test_select_group_ties_and_finished():
    W = 2
    scores = np.array([-1.0, -1.0], np.float32)
    cl = np.array([[-0.5, -2.0], [-0.5, -3.0]], np.float32)
    ci = np.array([[5, 6], [4, 7]])
    sl = np.array([[-0.25], [-9.0]], np.float32)
    tok, par, sc, fin = beam.select_group(scores, cl, ci, sl, np.array([9]), W)
    # order: stop (beam 0, -1.25), (0, 5, -1.5), (1, 4, -1.5): tie -> lower beam first
    assert fin == [(0, 9, np.float32(-1.25))]
    assert tok.tolist() == [5, 4] and par.tolist() == [0, 1] and sc.tolist() == [-1.5, -1.5]
    tok, par, sc, fin = beam.select_group(scores, cl, ci, sl, np.array([9]), W, first=True)
    assert tok.tolist() == [5, 6] and par.tolist() == [0, 0] and fin == [(0, 9, np.float32(-0.25))]


def test_results_length_penalty_and_ties():
    W = 2
    hist = np.array([[[3, 0], [4, 0]], [[5, 0], [6, 1]]])
    fins = [[(1, 1, 9, np.float32(-2.0))]]
    got = beam.results(hist, fins, [np.array([-2.0, -3.0], np.float32)], 1, W, 1.0)[0]
    # (3, 5) at -1.0 and (4, 9) at -1.0 tie: the finished entry of the same step was recorded first
    assert [t.tolist() for t, _ in got] == [[4, 9], [3, 5]] and [s for _, s in got] == [-1.0, -1.0]
    got = beam.results(hist, fins, [np.array([-2.0, -3.0], np.float32)], 1, W, 0.0)[0]
    assert [s for _, s in got] == [-2.0, -2.0]
    got = beam.results(hist[:1], [[(0, 0, 9, np.float32(-0.5))]], [np.array([-1.0, -1.5], np.float32)], 0, W, 2.0)[0]
    assert [t.tolist() for t, _ in got] == [[9], [3]]


# -- identities on the cpu device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("stops", [(), (3, 17, 40)])
def test_one_beam_is_generate_ragged(stops):
    prompts = _prompts([3, 1, 6, 2], seed=1)
    n = 9
    ref = _eval(_model("cpu"), lambda: np.stack([t.numpy().reshape(-1) for t in
                                                 _model_gen(prompts, n, stops)], 1))
    got = _beam(_model("cpu"), prompts, n, 1, stop_ids=stops)
    for g, hyps in enumerate(got):
        row = ref[g].tolist()
        hit = next((i for i, t in enumerate(row) if t in stops), None)
        want = row if hit is None else row[:hit + 1]
        assert len(hyps) == 1 and hyps[0][0].tolist() == want, (g, hyps, want)


def _model_gen(prompts, n, stops):
    m = _model("cpu")
    m.eval()
    out = list(m.generate_ragged(prompts, n, stop_ids=stops))
    while len(out) < n:                                   # (every row stopped: pad with -1 as a stopped row yields)
        out.append(type(out[0])(np.full((len(prompts), 1), -1, np.int64)))
    return out


def test_exhaustive_top_w_of_all_two_token_sequences():
    """V = 16, n = 2, W = 16 = V ** (n - 1): the result is the exact top 16 of all 256 sequences, scored from the model's
    own logits (the statement's float32 sums)."""
    Vs, W = 16, 16
    m = _model("cpu", B=W, vocab=Vs, seed=7)
    prompt = _prompts([4], seed=2, vocab=Vs)
    got = _beam(m, prompt, 2, W, length_penalty=0.0)[0]
    ref = _model("cpu", B=Vs, vocab=Vs, seed=7)
    m.eval()
    z0 = _eval(ref, lambda: ref._prefill_rows(prompt, np.array([0])).numpy())
    lp0 = beam.log_softmax_rows(z0)[0]
    pos = np.full(Vs, prompt[0].size + 1)
    for c in (c for layer in ref.layers for c in (layer.attention.cache_k, layer.attention.cache_v)):
        c.data[1:Vs, :prompt[0].size + 1] = c.data[0, :prompt[0].size + 1]
    from pydynet_amd.core import Tensor
    z1 = _eval(ref, lambda: ref._step_logits_rows(Tensor(np.arange(Vs).reshape(Vs, 1), dtype=np.int64), pos).numpy())
    lp1 = beam.log_softmax_rows(z1)
    seqs = [((np.float32(lp0[a]) + lp1[a, b]).astype(np.float32), a, b) for a, b in itertools.product(range(Vs), range(Vs))]
    seqs.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
    assert [t.tolist() for t, _ in got] == [[a, b] for _, a, b in seqs[:W]]
    assert [s for _, s in got] == [float(s) for s, _, _ in seqs[:W]]


def test_scores_are_normalised_and_sorted():
    prompts = _prompts([2, 5], seed=4)
    for lp in (0.0, 1.0, 2.5):
        got = _beam(_model("cpu"), prompts, 6, 3, length_penalty=lp, stop_ids=(1, 2, 3, 4, 5, 6))
        for hyps in got:
            assert len(hyps) == 3
            sc = [s for _, s in hyps]
            assert sc == sorted(sc, reverse=True)
            for toks, s in hyps:
                assert 1 <= toks.size <= 6 and toks.dtype == np.int64
                assert toks.size == 6 or toks[-1] in (1, 2, 3, 4, 5, 6)


@pytest.mark.parametrize("args, kw, msg", [
    (([[1, 2]], 4, 0), {}, "num_beams"), (([[1, 2]], 4, 17), {}, "num_beams"), (([[1, 2]], 4, 2.5), {}, "num_beams"),
    (([[1, 2]], 0, 2), {}, "max_new_tokens"), (([[1, 2]] * 3, 4, 3), {}, "max_batch_size"),
    (([[1, 64]], 4, 2), {}, "token ids"), (([[]], 4, 2), {}, "empty"), (([[1] * 30], 4, 2), {}, "outside"),
    (([[1, 2]], 4, 2), {"stop_ids": [64]}, "stop ids"), (([[1, 2]], 4, 2), {"stop_ids": range(17)}, "at most 16"),
    (([], 4, 2), {}, "at least one"), (([[1, 2]], 4, 2), {"length_penalty": float("nan")}, "length_penalty"),
])
def test_argument_errors(args, kw, msg):
    m = _model("cpu")
    with pytest.raises(ValueError, match=msg):
        _beam(m, *args, **kw)


def test_vocabulary_minus_stops_must_cover_the_beams():
    m = _model("cpu", B=16, vocab=16)
    with pytest.raises(ValueError, match="fewer than num_beams"):
        _beam(m, [[1, 2]], 3, 8, stop_ids=range(9))


# -- the emulated fast path == the cpu device, exactly ----------------------------------------------------------------
CASES = [([3, 1, 6], 2, (), 7), ([2, 5], 4, (7, 11, 30), 8), ([4], 8, (5,), 6), ([1, 4, 2], 4, (9, 20), 7)]


@pytest.mark.parametrize("fused", [2, 1, 0])
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_emulated_fast_path_matches_cpu(emulated_hip, monkeypatch, fused, graph, case):
    Graph.clear()
    lens, W, stops, n = CASES[case]
    prompts = _prompts(lens, seed=case)
    B = max(8, len(lens) * W)
    want = _beam(_model("cpu", B=B), prompts, n, W, stop_ids=stops, length_penalty=0.7)
    monkeypatch.setattr(Llama, "fused_decode", fused)
    monkeypatch.setattr(Llama, "graph_decode", graph)
    m = _model("hip:0", B=B)
    counters()
    got = _beam(m, prompts, n, W, stop_ids=stops, length_penalty=0.7)
    c = counters()
    _same(got, want)
    assert c[32] >= 3 and m._decode_st["beam"] == W
    assert m._decode_st["wide"] == (len(lens) * W > 8)


def test_emulated_generic_step_matches_cpu(emulated_hip, monkeypatch):
    """wide_decode = False past 8 rows: the generic per-row step, the beam launches one by one."""
    Graph.clear()
    lens, W, stops, n = CASES[3]
    prompts = _prompts(lens, seed=3)
    want = _beam(_model("cpu", B=12), prompts, n, W, stop_ids=stops)
    monkeypatch.setattr(Llama, "wide_decode", False)
    m = _model("hip:0", B=12)
    counters()
    got = _beam(m, prompts, n, W, stop_ids=stops)
    c = counters()
    _same(got, want)
    assert c[32] >= 3 * n - 2 and m._decode_st is None or not m._decode_st["ok"]


def test_groups_finish_at_different_steps(emulated_hip):
    """Many stop ids: groups end early and at different steps; the emulated path still equals the cpu device."""
    Graph.clear()
    prompts = _prompts([2, 3, 5, 1], seed=9)
    stops = tuple(range(0, 64, 5))
    want = _beam(_model("cpu"), prompts, 12, 2, stop_ids=stops)
    got = _beam(_model("hip:0"), prompts, 12, 2, stop_ids=stops)
    _same(got, want)
    ends = [max(t.size for t, _ in hyps) for hyps in want]
    assert len(set(ends)) > 1, ends


def test_greedy_generate_unchanged_around_beam_search(emulated_hip):
    Graph.clear()
    m = _model("hip:0")
    ids = np.random.default_rng(3).integers(0, V, (2, 4))

    def gen():
        return np.concatenate([t.numpy() for t in _eval(m, lambda: list(m.generate(ids, 12)))], 1)
    counters()
    before = gen()
    assert counters()[32] == 0
    _beam(m, _prompts([3, 2], seed=1), 5, 3)
    counters()
    after = gen()
    assert counters()[32] == 0
    assert np.array_equal(before, after)
