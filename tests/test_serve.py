"""Continuous batching (`Llama.serve` / `serve_all`: more requests than rows, a freed row refilled before the next step) on
the CPU: the `cpu` device (the module path) and the emulated C ABI with the slot entry points of
tests/abi_emulator/_decode_rows.py (the served graph-path plan at every fused level, without graphs, the generic HIP
step).  The contract: request r's tokens are the first budget_r tokens of row r of `generate_ragged` over all requests,
cut after its first stop id."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, margin

V = 64


def _model(dev, B=5, D=96, H=2, seq=32, seed=5):
    """head_dim 48 (D = 96, H = 2): the two-launch layer; H = 4: head_dim 24, the three-launch layer."""
    np.random.seed(seed)
    m = Llama(V, D, H, 96, seq, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(V, D).astype(np.float32)
    m.lm_head.weight.data[...] *= 8.0                  # logits of a few units: clear argmax margins, draws off the argmax
    return m.to(dev) if dev != "cpu" else m


def _eval(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn()
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _serve_all(m, prompts, budgets, **kw):
    return _eval(m, lambda: m.serve_all(prompts, budgets, **kw))


def _stream(m, prompts, budgets, **kw):
    return _eval(m, lambda: [(r.copy(), t.copy()) for r, t in m.serve(prompts, budgets, **kw)])


def _reference(prompts, budgets, H=2, **kw):
    """generate_ragged over every request on the `cpu` device (max_batch_size = N), with each step's logits."""
    m = _model("cpu", B=len(prompts), H=H)
    seen = []
    fwd = m.lm_head.forward

    def rec(x):
        y = fwd(x)
        seen.append(np.asarray(y.numpy())[:, -1, :])
        return y
    m.lm_head.forward = rec
    n = int(max(budgets))
    try:
        toks = _eval(m, lambda: np.stack([t.numpy().reshape(-1) for t in m.generate_ragged(prompts, n, **kw)], 1))
    finally:
        del m.lm_head.forward
    return toks, seen


def _want(ref, budgets, stops=()):
    out = []
    for r, n in enumerate(budgets):
        row = ref[r, :n].tolist()
        hit = next((i for i, t in enumerate(row) if t in stops), None)
        out.append(np.array(row if hit is None else row[:hit + 1], np.int64))
    return out


def _check(got, want, ref_logits, prompts, kw, exact):
    """Equal tokens; where the admitted prompt batches differ from the reference run's (`exact` False) a request may
    differ from its first differing token on, if that token's float64 margin in the reference is below 1e-5."""
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        if exact or np.array_equal(g, w):
            assert np.array_equal(g, w), (r, g, w)
            continue
        s = int(np.flatnonzero(g[:min(len(g), len(w))] != w[:min(len(g), len(w))])[0])
        z = ref_logits[s][r]
        if kw.get("temperature", 0) > 0:
            mg = margin(z, len(prompts[r]) + s, r, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw["seed"])
        else:
            srt = np.sort(z.astype(np.float64))
            mg = srt[-1] - srt[-2]
        assert mg < 1e-5, (r, s, mg)


def _prompts(lens, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, V, n) for n in lens]


SAMPLED = [dict(temperature=1.0, seed=3), dict(temperature=0.8, top_p=0.9, seed=11),
           dict(temperature=1.3, top_k=5, top_p=0.95, seed=2 ** 64 - 1)]
LENS, BUDGETS = [3, 1, 7, 2, 5], [4, 9, 0, 6, 3]


@pytest.mark.parametrize("slots", [1, 2, 3, 5])
@pytest.mark.parametrize("kw", [{}] + SAMPLED)
def test_serve_matches_generate_ragged_on_cpu(slots, kw):
    prompts = _prompts(LENS, seed=1)
    ref, logits = _reference(prompts, BUDGETS, **kw)
    got = _serve_all(_model("cpu"), prompts, BUDGETS, slots=slots, **kw)
    _check(got, _want(ref, BUDGETS), logits, prompts, kw, exact=slots >= len(prompts))
    assert len(got[2]) == 0                                       # a budget of 0: nothing


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("slots", [1, 2, 3, 5])
@pytest.mark.parametrize("kw", [{}] + SAMPLED[1:])
def test_serve_matches_generate_ragged_emulated(emulated_hip, H, slots, kw):
    Graph.clear()
    prompts = _prompts(LENS, seed=2)
    ref, logits = _reference(prompts, BUDGETS, H=H, **kw)
    m = _model("hip:0", H=H)
    counters()
    got = _serve_all(m, prompts, BUDGETS, slots=slots, **kw)
    c = counters()
    _check(got, _want(ref, BUDGETS), logits, prompts, kw, exact=slots >= len(prompts))
    assert c[30] > 0 and c[29] > 0                               # the slot ticks / store and the per-row step ran
    assert m._decode_st["serve"] and m._decode_st["ragged"] and m._decode_st["B"] == slots


@pytest.mark.parametrize("dev", ["cpu", "hip:0"])
@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
def test_more_requests_than_rows(emulated_hip, dev, kw):
    """N = 11 > max_batch_size = 4; the reference is one generate_ragged run on a model with 11 cache rows."""
    Graph.clear()
    lens = [1 + (5 * i) % 9 for i in range(11)]
    budgets = [(3 * i) % 8 for i in range(11)]                    # 0 .. 7, two zeros
    prompts = _prompts(lens, seed=3)
    ref, logits = _reference(prompts, budgets, **kw)
    got = _serve_all(_model(dev, B=4), prompts, budgets, **kw)    # slots = min(N, max_batch_size) = 4
    _check(got, _want(ref, budgets), logits, prompts, kw, exact=False)
    assert [len(g) for g in got] == budgets                       # (no stop ids: every request uses its budget)


@pytest.mark.parametrize("dev", ["cpu", "hip:0"])
@pytest.mark.parametrize("kw", [{}, SAMPLED[0]])
def test_stop_ids(emulated_hip, dev, kw):
    Graph.clear()
    prompts = _prompts([3, 6, 2, 4, 5, 1], seed=9)
    budgets = [12] * 6
    ref, logits = _reference(prompts, budgets, **kw)
    stops = {int(ref[0, 2]), int(ref[2, 5])}                      # request 0 stops by its 3rd token, 2 by its 6th
    want = _want(ref, budgets, stops)
    for slots in (2, 6):
        got = _serve_all(_model(dev, B=6), prompts, budgets, slots=slots, stop_ids=stops, **kw)
        _check(got, want, logits, prompts, kw, exact=slots == 6)
        assert len(got[0]) <= 3 and got[0][-1] in stops


def _schedule(budgets, lengths, S):
    """The stated schedule, restated: per step the lowest free row takes the lowest waiting request (budget > 0); a row
    frees after its request's last token.  `lengths[r]`: the number of tokens request r yields."""
    queue = [r for r in range(len(budgets)) if budgets[r] > 0]
    rows, done = [-1] * S, [0] * len(budgets)
    steps = []
    while queue or any(r >= 0 for r in rows):
        for b in range(S):
            if rows[b] < 0 and queue:
                rows[b] = queue.pop(0)
        steps.append(list(rows))
        for b in range(S):
            r = rows[b]
            if r >= 0:
                done[r] += 1
                if done[r] == lengths[r]:
                    rows[b] = -1
    return steps


@pytest.mark.parametrize("dev", ["cpu", "hip:0"])
def test_admission_order_and_stream(emulated_hip, dev):
    Graph.clear()
    prompts = _prompts([2, 4, 1, 3, 6, 2, 5], seed=4)
    budgets = [5, 1, 3, 0, 7, 2, 4]
    free = _serve_all(_model(dev, B=3), prompts, budgets)
    stops = {int(free[4][1])}
    for kw in ({}, {"stop_ids": stops}):
        m = _model(dev, B=3)
        toks = _serve_all(m, prompts, budgets, **kw)
        stream = _stream(_model(dev, B=3), prompts, budgets, **kw)
        steps = _schedule(budgets, [len(t) for t in toks], 3)
        assert [r.tolist() for r, _ in stream] == steps
        seen = [[] for _ in prompts]
        for reqs, tk in stream:
            assert reqs.shape == tk.shape == (3,) and reqs.dtype == tk.dtype == np.int64
            assert np.array_equal(reqs < 0, tk < 0)               # an empty row produces nothing, a full one a token
            for r, t in zip(reqs, tk):
                if r >= 0:
                    seen[r].append(int(t))
        assert all(np.array_equal(s, t) for s, t in zip(seen, toks))
        if kw:
            assert any(len(t) and t[-1] in stops and len(t) < budgets[r] for r, t in enumerate(toks))


@pytest.mark.parametrize("dev", ["cpu", "hip:0"])
def test_admission_prefill_leaves_other_rows_alone(emulated_hip, dev):
    m = _model(dev, B=4)
    rng = np.random.default_rng(0)
    for layer in m.layers:
        for c in (layer.attention.cache_k, layer.attention.cache_v):
            c.data[...] = rng.standard_normal(c.shape).astype(np.float32)
    before = [np.array(c.numpy()) for l in m.layers for c in (l.attention.cache_k, l.attention.cache_v)]
    prompts = _prompts([5, 2], seed=6)
    counters()
    first = _eval(m, lambda: m._serve_prefill(prompts, np.array([3, 1]), np.array([7, 2]), None))
    if dev != "cpu":
        assert counters()[30] >= 1
    after = [np.array(c.numpy()) for l in m.layers for c in (l.attention.cache_k, l.attention.cache_v)]
    for k0, k1 in zip(before, after):
        for b in (0, 2):                                          # rows that took no request: bit-identical
            assert np.array_equal(k0[b], k1[b])
        for b, n in ((3, 5), (1, 2)):
            assert not np.array_equal(k0[b, :n], k1[b, :n])       # the prompt's keys / values
            assert not k1[b, n].any()                             # the slot no decode step writes: zero
            assert np.array_equal(k0[b, n + 1:], k1[b, n + 1:])   # pad positions and beyond: untouched
    # the same keys / values and first tokens as one prompt pass of each prompt alone
    for i, (b, p) in enumerate(zip((3, 1), prompts)):
        one = _model("cpu", B=1)
        logits = _eval(one, lambda: one(p[None], 0).numpy()[0, -1])
        assert first[i] == int(np.argmax(logits))
        ref = [np.array(c.numpy()) for l in one.layers for c in (l.attention.cache_k, l.attention.cache_v)]
        for k1, r in zip(after, ref):
            np.testing.assert_allclose(k1[b, :len(p)], r[0, :len(p)], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["fused1", "unfused", "nograph", "module", "generic"])
@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
def test_every_path_emulated(emulated_hip, mode, kw):
    Graph.clear()
    n_req, rows = (12, 10) if mode == "generic" else (7, 3)       # generic: 10 slots > 8, the plan refuses
    prompts = _prompts([1 + (3 * i) % 7 for i in range(n_req)], seed=8)
    budgets = [2 + (5 * i) % 9 for i in range(n_req)]
    cpu = _serve_all(_model("cpu", B=rows), prompts, budgets, **kw)
    Llama.fused_decode = {"fused1": 1, "unfused": 0}.get(mode, 2)
    Llama.graph_decode = mode != "nograph"
    Llama.fast_decode = mode != "module"
    Llama.wide_decode = mode != "generic"                         # (generic: not the wide step either)
    try:
        m = _model("hip:0", B=rows)
        counters()
        got = _serve_all(m, prompts, budgets, **kw)
        c = counters()
    finally:
        Llama.fused_decode, Llama.graph_decode, Llama.fast_decode, Llama.wide_decode = 2, True, True, True
    assert all(np.array_equal(g, w) for g, w in zip(got, cpu))
    if mode == "generic":
        assert c[29] > 0 and m._decode_st["B"] == rows and not m._decode_st["ok"]
    if mode != "module":
        assert c[30] > 0                                          # (at least the store)


@pytest.mark.parametrize("bad", [
    dict(prompts=[]),                                             # no request
    dict(prompts=[[1, 2], []]),                                   # an empty prompt
    dict(prompts=[[1, 64]]),                                      # an id outside [0, vocab)
    dict(prompts=[[1, -1]]),
    dict(prompts=[[1, 2]], stop_ids=[64]),                        # a stop id outside [0, vocab)
    dict(prompts=[[1, 2]], stop_ids=[-1]),
    dict(prompts=[[1, 2]], n=-1),                                 # budgets
    dict(prompts=[[1, 2]], n=2.5),
    dict(prompts=[[1, 2], [3]], n=[4]),                           # one budget for two prompts
    dict(prompts=[[1, 2], [3]], n=[4, -2]),
    dict(prompts=[[1, 2]], n=[True]),
    dict(prompts=[[1, 2]], slots=0),                              # slots outside [1, max_batch_size]
    dict(prompts=[[1, 2]] * 7, slots=6),
    dict(prompts=[[1, 2]], slots=1.5),
    dict(prompts=[[1] * 20, [2]], n=[13, 2]),                     # request 0's last position is 32 >= max_seq_len
    dict(prompts=[[1] * 33], n=1),                                # a prompt longer than the cache
    dict(prompts=[[1, 2]], temperature=-1.0),                     # sampling arguments (check_sampling_args)
    dict(prompts=[[1, 2]], top_p=0.0),
    dict(prompts=[[1, 2]], seed=-1),
])
def test_invalid_arguments_raise_before_anything_runs(emulated_hip, bad):
    m = _model("hip:0")
    counters()
    kw = dict(bad)
    prompts, n = kw.pop("prompts"), kw.pop("n", 4)
    with pytest.raises(ValueError):
        m.serve(prompts, n, **kw)                                 # (not iterated: the call itself refuses)
    with pytest.raises(ValueError):
        m.serve_all(prompts, n, **kw)
    assert not any(counters())
    assert getattr(m, "_decode_st", None) is None


def test_bounds_are_per_request(emulated_hip):
    m = _model("hip:0", B=2)
    got = _serve_all(m, [[1] * 20, [2], [3] * 31], [12, 30, 0])   # last positions 31 and 30; a budget of 0 is not bound
    assert [len(g) for g in got] == [12, 30, 0]


def test_generate_and_generate_ragged_never_use_the_slot_entries(emulated_hip):
    Graph.clear()
    m = _model("hip:0")
    ids = np.stack(_prompts([4, 4, 4], seed=6))
    counters()
    _eval(m, lambda: [t.numpy() for t in m.generate(ids, 14)])
    _eval(m, lambda: [t.numpy() for t in m.generate(ids, 14, **SAMPLED[0])])
    _eval(m, lambda: [t.numpy() for t in m.generate_ragged(_prompts([2, 6, 1], seed=2), 9, stop_ids=[3])])
    _eval(m, lambda: [t.numpy() for t in m.generate_ragged(_prompts([2, 6, 1], seed=2), 9, **SAMPLED[1])])
    assert counters()[30] == 0
    assert not m._decode_st["serve"]


def test_serve_then_ragged_then_serve(emulated_hip):
    """One model, three runs: serve re-plans with its own key (a serve plan never shares a plan or a graph)."""
    Graph.clear()
    prompts = _prompts([2, 6, 4, 3], seed=5)
    budgets = [6, 3, 8, 5]
    m = _model("hip:0")
    a = _serve_all(m, prompts, budgets, slots=2)
    key = m._decode_st["key"]
    assert key[-1] is True and m._decode_st["serve"]
    _eval(m, lambda: [t.numpy() for t in m.generate_ragged(prompts, 5)])
    assert m._decode_st["key"][-1] is False and not m._decode_st["serve"]
    b = _serve_all(m, prompts, budgets, slots=2)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_abandoned_serve_then_a_new_one(emulated_hip):
    Graph.clear()
    prompts = _prompts([2, 6, 4, 3, 5], seed=7)
    m = _model("hip:0")
    want = _serve_all(_model("hip:0"), prompts, 9, slots=2)
    m.eval()
    it = m.serve(prompts, 9, slots=2)
    for _ in range(4):
        next(it)
    it.close()
    m.train(True)
    assert all(np.array_equal(x, y) for x, y in zip(_serve_all(m, prompts, 9, slots=2), want))


def test_sample_next_rows_counter_ids():
    from pydynet_amd.core import Tensor
    z = np.random.default_rng(0).standard_normal((3, 40)).astype(np.float32) * 3
    pos = np.array([5, 9, 2])
    dflt = sampling.sample_next_rows(Tensor(z), pos, 0.9, seed=4).numpy().reshape(-1)
    assert np.array_equal(dflt, sampling.sample_next_rows(Tensor(z), pos, 0.9, seed=4, rows=[0, 1, 2]).numpy().reshape(-1))
    got = sampling.sample_next_rows(Tensor(z), pos, 0.9, seed=4, rows=[7, 0, 11]).numpy().reshape(-1)
    want = [sampling.sample_rows_np(z[b:b + 1], int(pos[b]), 0.9, seed=4, rows=[r])[0] for b, r in enumerate([7, 0, 11])]
    assert np.array_equal(got, want)
