"""allowed_token_ids, logit_bias and min_new_tokens (`generate`, `generate_ragged`, `serve`, `serve_all`) on the CPU: the
statement of llm/logit_edits.py by hand cases, argument errors, the packed forms, and the emulated C ABI with the entry
points of tests/abi_emulator/_logitedit.py (the graph-replayed steps, with and without graphs) against `cpu`."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import logit_edits as E
from pydynet_amd.llm import penalties
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, remove
from tests.abi_emulator import _logitedit
from tests.test_ragged import SAMPLED, V, _gen, _model, _prompts, _ragged

f32 = np.float32
INF = np.inf
PEN = dict(repetition_penalty=1.8, presence_penalty=0.7, frequency_penalty=0.4)


# -- the statement ----------------------------------------------------------------------------------------------------
def test_allowed_set_bans_everything_else():
    z = np.array([[2.0, -1.0, 3.0, 0.5], [1.0, 2.0, 3.0, 4.0]], f32)
    got = E.apply(z, [np.array([1, 3]), None])
    assert got.tolist() == [[-INF, -1.0, -INF, 0.5], [1.0, 2.0, 3.0, 4.0]]
    assert got.dtype == np.float32 and z[0, 0] == 2.0            # (a new array)


def test_bias_is_one_float32_addition():
    rng = np.random.default_rng(0)
    z = (7 * rng.standard_normal((3, 50))).astype(f32)
    ids = [rng.permutation(50)[:9] for _ in range(3)]
    vals = [(5 * rng.standard_normal(9)).astype(f32) for _ in range(3)]
    got = E.apply(z, None, list(zip(ids, vals)))
    want = z.copy()
    for b in range(3):
        for i, v in zip(ids[b], vals[b]):
            want[b, i] = f32(z[b, i]) + f32(v)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(E.apply(z, None, [dict(zip(i.tolist(), v.tolist())) for i, v in zip(ids, vals)]), want)


def test_zeros_infinities_and_the_ban():
    z = np.array([[0.0, -0.0, INF, -INF, INF, 1.0, -0.0]], f32)
    bias = [(np.arange(7), np.array([-0.0, -0.0, 3.0, 5.0, -INF, -INF, 0.0], f32))]
    got = E.apply(z, None, bias)[0]
    assert got[0] == 0.0 and not np.signbit(got[0])              # +0 + -0 = +0
    assert got[1] == 0.0 and np.signbit(got[1])                  # -0 + -0 = -0
    assert got[2] == INF and got[3] == -INF                      # infinities stay under a finite bias
    assert got[4] == -INF                                        # beta = -inf on a +inf logit: an assignment, not NaN
    assert got[5] == -INF
    assert got[6] == 0.0 and not np.signbit(got[6])              # -0 + +0 = +0
    assert not np.isnan(got).any()


def test_bias_cannot_revive_a_token_outside_the_allowed_set():
    z = np.array([[1.0, 2.0, 3.0]], f32)
    got = E.apply(z, [np.array([0, 1])], [{2: 1e30, 0: 0.5}])
    assert got.tolist() == [[1.5, 2.0, -INF]]                    # allowed first, then the bias: -inf + 1e30 = -inf


def test_min_new_tokens_boundary():
    z = np.tile(np.array([1.0, 5.0, 2.0, 4.0], f32), (4, 1))
    got = E.apply(z, None, None, generated=np.array([0, 2, 3, 7]), m=3, stop_ids=[1, 3])
    assert got[0].tolist() == [1.0, -INF, 2.0, -INF] and got[1].tolist() == [1.0, -INF, 2.0, -INF]
    assert got[2].tolist() == [1.0, 5.0, 2.0, 4.0] and got[3].tolist() == [1.0, 5.0, 2.0, 4.0]     # t - s_b = m: free
    assert np.array_equal(E.apply(z, m=0, stop_ids=[1]), z) and np.array_equal(E.apply(z, m=2, stop_ids=[]), z)
    assert E.apply(z[:1], m=1, stop_ids=[0])[0, 0] == -INF       # (generated None: 0)
    # a bias on a stop id does not lift the ban: the ban comes last
    assert E.apply(z[:1], None, [{1: 100.0}], [0], 1, [1])[0, 1] == -INF


def test_order_against_the_penalties():
    """The edits run on the penalised row: penalise, then add the bias -- not the other way round."""
    z = np.array([[4.0, -2.0, 1.0]], f32)
    c = np.array([[2, 0, 0]])
    seen = np.array([[False, True, False]])
    pen = penalties.penalize(z, c, seen, 2.0, 0.5, 0.25)
    got = E.apply(pen, None, [{0: 3.0, 1: 3.0}])
    assert got.tolist() == [[(4.0 / 2.0 - (0.25 * 2 + 0.5)) + 3.0, -2.0 * 2.0 + 3.0, 1.0]]
    other = penalties.penalize(E.apply(z, None, [{0: 3.0, 1: 3.0}]), c, seen, 2.0, 0.5, 0.25)
    assert not np.array_equal(got, other)


def test_rows_state():
    spec = E.check_args([{3: -INF}, None, {1: 2.0}], [None, [0, 1, 2], None], 2, V=6, n=3, stop_ids=[0])
    rows = E.Rows(2, spec)
    z = np.zeros((2, 6), f32)
    assert np.array_equal(rows.apply(z, [4, 4]), z)              # no request in the rows yet
    rows.reset([1, 0], [0, 2], [3, 5])
    got = rows.apply(z, [6, 4])                                  # row 0: request 2, generated 1; row 1: request 0, generated 1
    assert got[0].tolist() == [-INF, 2.0, 0, 0, 0, 0] and got[1].tolist() == [-INF, 0, 0, -INF, 0, 0]
    got = rows.apply(z, [7, -1])                                 # row 0 past min_new_tokens, row 1 computes nothing
    assert got[0].tolist() == [0, 2.0, 0, 0, 0, 0] and got[1].tolist() == [0] * 6
    assert rows.apply(z[1:], [3], rows=[1])[0].tolist() == [-INF, 0, 0, -INF, 0, 0]


# -- arguments --------------------------------------------------------------------------------------------------------
def test_defaults_are_off():
    assert E.check_args(V=10, n=3) is None
    assert E.check_args(None, None, 0, 10, 3, stop_ids=[2], speculate=4) is None
    assert E.check_args([None, None], [None, None], 0, 10, 2) is None
    spec = E.check_args({3: 1.5, 1: -INF}, None, 0, 10, 2)
    assert spec.m == 0 and len(spec.reqs) == 2 and spec.reqs[1][0] is None
    assert spec.reqs[0][1].tolist() == [1, 3] and spec.reqs[0][2].tolist() == [-INF, 1.5]        # sorted by id
    spec = E.check_args(None, [[4, 2, 2], None, np.array([7])], 0, 10, 3)
    assert spec.reqs[0][0].tolist() == [2, 4] and spec.reqs[1][0] is None and spec.reqs[2][0].tolist() == [7]
    assert E.check_args(None, (5, 6), 0, 10, 2).reqs[1][0].tolist() == [5, 6]                   # one set for the call
    assert E.check_args(None, None, 3, 10, 1, stop_ids=[4]).m == 3
    assert E.check_args({0: -1e30}, None, 0, 10, 1).reqs[0][2][0] == f32(-1e30)


BAD = [dict(logit_bias={10: 1.0}), dict(logit_bias={-1: 1.0}), dict(allowed_token_ids=[0, 10]),
       dict(allowed_token_ids=[-1]),                                                     # ids outside [0, V)
       dict(logit_bias={1.5: 1.0}), dict(logit_bias={"3": 1.0}), dict(logit_bias={True: 1.0}),
       dict(allowed_token_ids=[1.0, 2.0]), dict(allowed_token_ids=np.array([1.0])),      # non-integer ids
       dict(allowed_token_ids=[]), dict(allowed_token_ids=[[1], []]),                    # an empty allowed set
       dict(logit_bias={3: float("nan")}), dict(logit_bias={3: INF}), dict(logit_bias={3: 1e39}),
       dict(logit_bias={3: -1e39}), dict(logit_bias={3: "1"}), dict(logit_bias={3: None}),
       dict(logit_bias=[1.0, 2.0]), dict(logit_bias=[{1: 1.0}]), dict(allowed_token_ids=[[1], [2], [3]]),
       dict(min_new_tokens=-1, stop_ids=[1]), dict(min_new_tokens=1.5, stop_ids=[1]),
       dict(min_new_tokens=True, stop_ids=[1]), dict(min_new_tokens=2),                  # m > 0 without stop ids
       dict(allowed_token_ids=[3, 4], logit_bias={3: -INF, 4: -INF}),                    # nothing left to pick
       dict(allowed_token_ids=[3, 4], logit_bias={3: -INF}, min_new_tokens=1, stop_ids=[4]),
       dict(allowed_token_ids=[[1], [2, 5]], min_new_tokens=1, stop_ids=[1]),
       dict(logit_bias={v: -INF for v in range(10)})]


@pytest.mark.parametrize("bad", BAD)
def test_bad_arguments_raise(bad):
    with pytest.raises(ValueError):
        E.check_args(V=10, n=2, **bad)


def test_too_many_bias_entries_and_speculation():
    with pytest.raises(ValueError, match="MAX_BIAS"):
        E.check_args({v: 0.5 for v in range(E.MAX_BIAS + 1)}, V=5000, n=1)
    assert E.check_args({v: 0.5 for v in range(E.MAX_BIAS)}, V=5000, n=1).reqs[0][1].size == E.MAX_BIAS == 1024
    with pytest.raises(ValueError, match="speculate"):
        E.check_args({1: 1.0}, V=10, n=1, speculate=2)
    m = _model("cpu")
    with pytest.raises(ValueError, match="speculate"):
        m.generate_ragged(_prompts([2, 3]), 4, speculate=2, allowed_token_ids=[1, 2])
    m.generate_ragged(_prompts([2, 3]), 4, speculate=2, logit_bias=None, allowed_token_ids=None, min_new_tokens=0)


@pytest.mark.parametrize("bad", [dict(logit_bias={V: 1.0}), dict(allowed_token_ids=[]), dict(logit_bias={1: INF}),
                                 dict(allowed_token_ids=[[1], [2], [3]])])
def test_bad_arguments_raise_before_any_launch(emulated_hip, bad):
    from pydynet_amd import _lib
    _logitedit.extend()
    m = _model("hip:0")
    prompts = _prompts([2, 3])
    n0 = len(_lib._LIB.calls)
    for call in (lambda: m.generate(np.stack(_prompts([3, 3])), 8, **bad),
                 lambda: m.generate_ragged(prompts, 4, **bad),
                 lambda: m.serve(prompts, 4, **bad),
                 lambda: m.serve(prompts, 4, prefill_chunk=2, **bad),
                 lambda: m.serve_all(prompts, 4, **bad),
                 lambda: m.serve_all(prompts, 4, min_new_tokens=2),
                 lambda: m.generate_ragged(prompts, 4, min_new_tokens=-1, stop_ids=[1])):
        with pytest.raises(ValueError):
            call()
    assert len(_lib._LIB.calls) == n0
    with pytest.raises(TypeError):
        m.generate(np.stack(_prompts([3, 3])), 8, min_new_tokens=1)       # (generate has no stop ids)


# -- the packed forms -------------------------------------------------------------------------------------------------
def test_packed_forms_round_trip():
    rng = np.random.default_rng(3)
    Vv = 1001                                                    # a partial last word
    allow = [np.sort(rng.permutation(Vv)[:n]) if n else None for n in (1, 0, 1000, 37)]
    allow[0] = np.array([Vv - 1])
    bits, on = E.allow_bits(allow, Vv)
    assert bits.shape == (4, 32) and bits.dtype == np.int32 and on.tolist() == [1, 0, 1, 1] and not bits[1].any()
    back = E.bits_allow(bits, on, Vv)
    assert back[1] is None and all(np.array_equal(a, b) for a, b in zip(allow, back) if a is not None)
    assert bits.view(np.uint32)[0, 31] == 1 << ((Vv - 1) & 31)
    bias = [(rng.permutation(5000)[:n].astype(np.int32), rng.standard_normal(n).astype(f32)) for n in (0, 1, E.MAX_BIAS)]
    bias[1][1][0] = -INF
    ids, vals, cnt = E.bias_tables(bias + [None])
    assert ids.shape == vals.shape == (4, E.MAX_BIAS) and cnt.tolist() == [0, 1, E.MAX_BIAS, 0]
    assert (np.diff(ids[2]) > 0).all()                           # sorted by id
    for (i, v), (bi, bv) in zip(bias, E.tables_bias(ids, vals, cnt)):
        o = np.argsort(i)
        assert np.array_equal(bi, i[o]) and np.array_equal(bv, v[o])
    assert E.params_bytes(5).view(np.int32).tolist() == [5, 0, 0, 0] and E.params_bytes(5).dtype == np.int64
    spec = E.check_args([{2: 1.0}, None], [None, None], 0, Vv, 2)
    p = spec.packed([1, 0, 0])
    assert p[0] is None and p[1] is None and p[4].tolist() == [0, 1, 1] and p[2][1, 0] == 2
    assert E.check_args(None, [[1], None], 0, Vv, 2).packed([0])[0] is not None


# -- the emulated HIP path --------------------------------------------------------------------------------------------
def _edits(N, vocab=V, seed=0):
    """Per-request edits: request r has a bias (a ban, a strong push and small shifts), an allowed set, both or neither."""
    rng = np.random.default_rng(seed)
    bias, allow = [], []
    for r in range(N):
        ids = rng.permutation(vocab)[:8]
        b = {int(t): float(v) for t, v in zip(ids, rng.standard_normal(8) * 3)}
        b[int(ids[0])] = -INF
        b[int(ids[1])] = 6.0
        a = np.sort(rng.permutation(vocab)[:max(3, vocab // 4)])
        a[0] = ids[1]                                            # (never empty after the ban)
        bias.append(b if r % 4 in (0, 2) else None)
        allow.append(a.tolist() if r % 4 in (1, 2) else None)
    return dict(logit_bias=bias, allowed_token_ids=allow)


def _rows(a):
    return [[int(t) for t in r[:np.argmax(r < 0)]] if (r < 0).any() else [int(t) for t in r] for r in a]


def _serve_all(m, prompts, budgets, **kw):
    m.eval()
    try:
        with pdn.no_grad():
            return m.serve_all(prompts, budgets, **kw)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _with_lp(m, it):
    """A run with logprobs: (tokens (B, steps), token logprobs, top ids (B, steps, n), top logprobs)."""
    m.eval()
    try:
        with pdn.no_grad():
            steps = [(t.numpy().reshape(-1).copy(), lp) for t, lp in it]
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
    return (np.stack([s[0] for s in steps], 1), np.stack([np.asarray(s[1].token).reshape(-1) for s in steps], 1),
            np.stack([s[1].top_ids for s in steps], 1), np.stack([s[1].top_logprobs for s in steps], 1))


def _check_properties(toks, ed, r):
    toks = [t for t in toks if t >= 0]
    b, a = ed["logit_bias"][r], ed["allowed_token_ids"][r]
    if b is not None:
        assert not {t for t, v in b.items() if v == -INF} & set(toks), r         # a banned token never appears
    if a is not None:
        assert set(toks) <= set(a), r                                            # every token lies in the allowed set


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (5, SAMPLED[1]), (12, {}), (10, SAMPLED[0])])
def test_emulated_generate_ragged_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    _logitedit.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    prompts = _prompts([1 + (3 * i) % 7 for i in range(B)], seed=12)
    ed = _edits(B, seed=B)
    plain = _ragged(_model("cpu", B=max(B, 5)), prompts, 9, **kw)
    stop = int(plain[0, 1])
    kw = dict(kw, stop_ids=[stop], min_new_tokens=4, **ed)
    want = _ragged(_model("cpu", B=max(B, 5)), prompts, 9, **kw)
    m = _model("hip:0", B=max(B, 5))
    counters(49)
    got = _ragged(m, prompts, 9, **kw)
    c = counters(49)
    assert np.array_equal(got, want) and not np.array_equal(got, plain[:, :got.shape[1]])
    st = m._decode_st
    # one reset for the run, one launch per decode step and one for the prompt pass
    assert st["edit"] and st["full"] and c[48] == got.shape[1] + 1 and c[35] == 0
    assert st["edit_start"].get().tolist() == [p.size for p in prompts]
    for r, toks in enumerate(_rows(got)):
        _check_properties(toks, ed, r)
        assert stop not in toks[:4], r                           # no row ends before min_new_tokens tokens


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (2, SAMPLED[2]), (12, {})])
def test_emulated_generate_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    _logitedit.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    ids = np.stack(_prompts([5] * B, seed=13))
    ed = _edits(B, seed=20 + B)
    want = _gen(_model("cpu", B=max(B, 5)), ids, 5 + 10, **kw, **ed)
    counters(49)
    got = _gen(_model("hip:0", B=max(B, 5)), ids, 5 + 10, **kw, **ed)
    assert np.array_equal(got, want) and counters(49)[48] == 11
    assert not np.array_equal(got, _gen(_model("cpu", B=max(B, 5)), ids, 5 + 10, **kw))
    for r, toks in enumerate(got.tolist()):
        _check_properties(toks, ed, r)
    # one value for the whole call
    one = dict(logit_bias={7: -INF, 9: 2.5}, allowed_token_ids=list(range(5, 40)))
    want = _gen(_model("cpu", B=max(B, 5)), ids, 5 + 6, **kw, **one)
    got = _gen(_model("hip:0", B=max(B, 5)), ids, 5 + 6, **kw, **one)
    assert np.array_equal(got, want) and 7 not in got and got.min() >= 5 and got.max() < 40


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("S,chunk,prefix,kw", [(3, None, False, {}), (3, 4, False, {}), (3, 4, True, {}),
                                                (2, None, False, SAMPLED[1]), (10, None, False, {}),
                                                (10, 3, True, SAMPLED[0])])
def test_emulated_serve_equals_cpu(emulated_hip, graphs, S, chunk, prefix, kw, monkeypatch):
    _logitedit.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    N = S + 4
    rng = np.random.default_rng(14)
    head = rng.integers(0, V, 3)                                 # (a shared start: the prefix cache has something to reuse)
    prompts = [np.concatenate([head, rng.integers(0, V, 1 + (5 * i) % 6)]) for i in range(N)]
    budgets = [2 + (3 * i) % 7 for i in range(N)]
    ed = _edits(N, seed=S)
    plain = _serve_all(_model("cpu", B=N), prompts, budgets, slots=S, prefill_chunk=chunk, **kw)
    stop = int(plain[2][1])
    kw = dict(kw, slots=S, stop_ids=[stop], min_new_tokens=3, prefill_chunk=chunk, prefix_cache=prefix, **ed)
    want = _serve_all(_model("cpu", B=N), prompts, budgets, **kw)
    counters(49)
    m = _model("hip:0", B=N)
    got = _serve_all(m, prompts, budgets, **kw)
    assert [g.tolist() for g in got] == [w.tolist() for w in want] and counters(49)[48] > 0
    assert m._decode_st["edit"]
    if prefix:
        assert m.prefix_stats["hits"] > 0
    for r, toks in enumerate(got):
        _check_properties(toks.tolist(), ed, r)
        assert stop not in toks.tolist()[:3] and (toks.size >= min(3, budgets[r])), r
    assert any(stop in p.tolist()[:3] for p in plain)            # the constraint bites: unedited, a request ends early


def test_emulated_with_penalties_and_logprobs(emulated_hip):
    """Penalties, edits and logprobs = 3 together: tokens and records as on `cpu`; a request restricted to two tokens
    reports -inf for the third of its top 3 (a banned token)."""
    _logitedit.extend()
    Graph.clear()
    for B in (4, 11):
        prompts = _prompts([1 + (3 * i) % 5 for i in range(B)], seed=31)
        ed = _edits(B, seed=31)
        ed["allowed_token_ids"][1], ed["logit_bias"][1] = [11, 40], None
        kw = dict(logprobs=3, **PEN, **ed)
        mc, mh = _model("cpu", B=B), _model("hip:0", B=B)
        want = _with_lp(mc, mc.generate_ragged(prompts, 8, **kw))
        counters(49)
        got = _with_lp(mh, mh.generate_ragged(prompts, 8, **kw))
        c = counters(49)
        assert c[48] == 9 and c[35] == 9 and mh._decode_st["edit"] and mh._decode_st["pen"]
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.allclose(got[1], want[1], rtol=1e-5, atol=1e-4) and np.allclose(got[3], want[3], rtol=1e-5, atol=1e-4)
        assert set(got[0][1].tolist()) <= {11, 40} and (got[3][1, :, 2] == -INF).all() and np.isfinite(got[3][1, :, :2]).all()
        assert not np.array_equal(got[0], _ragged(_model("cpu", B=B), prompts, 8, **PEN))
    # serve_all, plain and chunked with the prefix cache
    N = 7
    prompts = _prompts([3, 1, 6, 2, 4, 5, 2], seed=8)
    budgets = [6, 3, 9, 1, 7, 4, 8]
    ed = _edits(N, seed=5)
    ed["allowed_token_ids"][0], ed["logit_bias"][0] = [3, 50], None
    for chunk, prefix in ((None, False), (3, True)):
        kw = dict(slots=3, prefill_chunk=chunk, prefix_cache=prefix, logprobs=3, **PEN, **ed)
        want = _serve_all(_model("cpu", B=N), prompts, budgets, **kw)
        got = _serve_all(_model("hip:0", B=N), prompts, budgets, **kw)
        for (gt, gl), (wt, wl) in zip(got, want):
            assert np.array_equal(gt, wt) and np.array_equal(gl.top_ids, wl.top_ids)
            assert np.allclose(gl.token, wl.token, rtol=1e-5, atol=1e-4)
            assert np.allclose(gl.top_logprobs, wl.top_logprobs, rtol=1e-5, atol=1e-4)
        assert (got[0][1].top_logprobs[:, 2] == -INF).all() and set(got[0][0].tolist()) <= {3, 50}


def test_cpu_serve_all_equals_generate_ragged():
    """The serve promise holds with edits: request r's tokens are row r's of generate_ragged, whichever row it runs in."""
    prompts = _prompts([3, 1, 6, 2, 4, 5, 2], seed=8)
    budgets = [6, 3, 9, 1, 7, 4, 8]
    ed = _edits(7, seed=9)
    full = _ragged(_model("cpu", B=7), prompts, 9, **ed)
    for chunk in (None, 3):
        got = _serve_all(_model("cpu", B=7), prompts, budgets, slots=3, prefill_chunk=chunk, **ed)
        assert [g.tolist() for g in got] == [r[:b].tolist() for r, b in zip(full, budgets)]


def test_emulated_refusing_library_follows_the_statement(emulated_hip, monkeypatch):
    """Without the pdne_ entries (the emulator not extended) every path applies the statement on the host; and with
    the step entry removed the plan refuses likewise.  Tokens as on `cpu`."""
    from pydynet_amd import _lib
    prompts = _prompts([3, 6, 2], seed=15)
    ed = _edits(3, seed=15)
    want = _ragged(_model("cpu"), prompts, 9, **ed)
    budgets = [5, 7, 3]
    served = [w.tolist() for w in _serve_all(_model("cpu"), prompts, budgets, slots=2, **ed)]
    for extended in (False, True):
        Graph.clear()
        if extended:
            _logitedit.extend()
            remove(monkeypatch, _lib._LIB, "pdne_logit_edit_step_f32")
        assert not _lib.provides("pdne_logit_edit_step_f32")
        counters(49)
        m = _model("hip:0")
        got = _ragged(m, prompts, 9, **ed)
        c = counters(49)
        assert np.array_equal(got, want) and c[48] == 0 and c[29] > 0 and m._decode_st["ok"] is False
        assert [g.tolist() for g in _serve_all(_model("hip:0"), prompts, budgets, slots=2, **ed)] == served


def test_default_launches_unchanged(emulated_hip):
    """With the defaults the plan key, the launches and the counters are those of a run without the keywords."""
    from pydynet_amd import _lib
    _logitedit.extend()
    Graph.clear()
    ids = np.stack(_prompts([4, 4], seed=10))
    off = dict(logit_bias=None, allowed_token_ids=None)
    runtime = ("pdn_malloc", "pdn_free", "pdn_set_device", "pdn_compute_stream", "pdn_fill", "pdn_kernel_counters",
               "pdn_memcpy")                                   # (allocator / setup traffic differs between first uses)

    def run(fn):
        _lib._LIB.calls.clear()
        counters(49)
        out = fn()
        return out, counters(49), [c for c in _lib._LIB.calls if not c.startswith(runtime)]
    m0, m1 = _model("hip:0"), _model("hip:0")
    base, c0, calls0 = run(lambda: _gen(m0, ids, 14))
    again, c1, calls1 = run(lambda: _gen(m1, ids, 14, **off))
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[48] == 0
    assert not any("logit_edit" in c for c in calls0)
    k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
    assert len(k0) == len(k1) and "edit" not in k1 and m1._decode_st["edit"] is False
    assert "edit_allow" not in m1._decode_st
    prompts = _prompts([3, 5, 2], seed=11)
    m0, m1 = _model("hip:0"), _model("hip:0")
    base, c0, calls0 = run(lambda: _ragged(m0, prompts, 6, stop_ids=[5]))
    again, c1, calls1 = run(lambda: _ragged(m1, prompts, 6, stop_ids=[5], min_new_tokens=0, **off))
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[48] == 0
    assert len(m0._decode_st["key"]) == len(m1._decode_st["key"]) == len(k0)
    base, c0, calls0 = run(lambda: [o.tolist() for o in _serve_all(m0, prompts, 5, slots=2, prefill_chunk=2)])
    again, c1, calls1 = run(lambda: [o.tolist() for o in _serve_all(m1, prompts, 5, slots=2, prefill_chunk=2,
                                                                     min_new_tokens=0, **off)])
    assert base == again and c0 == c1 and calls0 == calls1 and c0[48] == 0
    # with an edit the key grows by one term, behind the logprobs term
    _ragged(m1, prompts, 6, logprobs=None, allowed_token_ids=[1, 2, 3])
    assert m1._decode_st["key"][-1] == "edit" and len(m1._decode_st["key"]) == len(k0) + 1


def test_emulated_entries_follow_the_statement(emulated_hip):
    """The emulated reset / step / rows entries through the library's call path: the statement on random rows."""
    from pydynet_amd import _lib, hipnp as hp
    _logitedit.extend()
    rng = np.random.default_rng(16)
    B, Vv = 4, 2500
    z = (5 * rng.standard_normal((B, Vv))).astype(f32)
    spec = E.check_args([{0: -INF, 1023: 2.0, 1024: -1.0, 2499: 3.0}, None, {5: 1.0}, None],
                        [None, [7, 1500, 2499], [5, 6], None], 2, Vv, 4, stop_ids=[6, 2000])
    bits, on, ids, vals, cnt = spec.packed([0, 1, 2, 3])
    pos, start = np.array([4, -1, 9, 2], np.int32), np.array([3, 1, 5, 2], np.int32)
    want = E.apply(z, spec.allow_rows(range(4)), spec.bias_rows(range(4)), pos - start, 2, [6, 2000])
    want[1] = z[1]
    assert want[0, 0] == -INF and want[0, 2000] == -INF and want[2, 7] == -INF and want[2, 5] == z[2, 5] + f32(1.0)
    assert want[2, 6] == z[2, 6]                                 # row 2 has generated 4 >= 2 tokens: its stop id is free
    assert want[3, 6] == -INF and want[3, 7] == z[3, 7]          # row 3: generated 0 < 2, nothing else
    stop = np.zeros(-(-Vv // 32), np.uint32)
    stop[6 >> 5] |= 1 << 6
    stop[2000 >> 5] |= np.uint32(1) << np.uint32(2000 & 31)
    L = _lib.lib()
    n = L.query("pdne_logit_edit_chunks", Vv)
    assert n == 3 and L.query("pdne_logit_edit_chunks", 0) == 0 and L.query("pdne_logit_edit_chunks", 1024) == 1
    # the reset into a zeroed state, rows permuted, one row outside
    st = [hp.zeros((B, bits.shape[1]), np.int32), hp.zeros((B,), np.int32), hp.zeros((B, E.MAX_BIAS), np.int32),
          hp.zeros((B, E.MAX_BIAS), np.float32), hp.zeros((B,), np.int32), hp.zeros((B,), np.int32)]
    order = np.array([2, 0, 9, 3, 1], np.int32)
    pick = np.array([2, 0, 0, 3, 1])
    src = [hp.asarray(np.ascontiguousarray(a[pick])) for a in (bits, on, ids, vals, cnt, start)]
    L.call("pdne_logit_edit_reset", *(a._ptr for a in st), B, Vv, hp.asarray(order)._ptr, 5, *(a._ptr for a in src),
           hp.stream())
    assert np.array_equal(st[1].get(), on) and np.array_equal(st[4].get(), cnt) and np.array_equal(st[5].get(), start)
    assert np.array_equal(st[0].get()[on > 0], bits[on > 0]) and np.array_equal(st[2].get(), ids)
    prm, x, P, S = (hp.asarray(a) for a in (E.params_bytes(2), z, pos, stop.view(np.int32)))
    cv, ci = hp.asarray(np.full((B, n), 7.0, f32)), hp.asarray(np.full((B, n), -7, np.int32))
    L.call("pdne_logit_edit_step_f32", x._ptr, Vv, B, Vv, prm._ptr, *(a._ptr for a in st), P._ptr, 1, S._ptr, cv._ptr,
           ci._ptr, hp.stream())
    assert np.array_equal(x.get().view(np.int32), want.view(np.int32))
    assert ci.get()[0].tolist() == [int(np.argmax(want[0, :1024])), 1024 + int(np.argmax(want[0, 1024:2048])),
                                    2048 + int(np.argmax(want[0, 2048:]))]
    assert (cv.get()[1] == 7.0).all() and (ci.get()[1] == -7).all() and cv.get()[2, 0] == want[2].max()
    # the rows form without any state: nothing changes; with the tables alone: the bias
    x = hp.asarray(z)
    L.call("pdne_logit_edit_rows_f32", x._ptr, Vv, B, Vv, prm._ptr, None, None, None, None, None, None, None, None, None,
           None, hp.stream())
    assert np.array_equal(x.get(), z)
    d = [hp.asarray(a) for a in (ids, vals, cnt)]
    L.call("pdne_logit_edit_rows_f32", x._ptr, Vv, B, Vv, prm._ptr, None, None, *(a._ptr for a in d), None, None, None,
           None, None, hp.stream())
    assert np.array_equal(x.get(), E.apply(z, None, spec.bias_rows(range(4))))
