"""token_fsm (`generate`, `generate_ragged`, `serve`, `serve_all`) on the CPU: the statement of llm/token_fsm.py by hand
cases, constructor and argument errors, the two constructors, the packed form, and the emulated C ABI with the entry points
of tests/abi_emulator/_fsm.py (the graph-replayed steps, with and without graphs) against `cpu`.  Every produced sequence
is walked through its machine in plain Python."""
import itertools

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import token_fsm as F
from pydynet_amd.llm.llama import Llama
from pydynet_amd.llm.token_fsm import TokenFSM
from tests.abi_emulator import counters, remove
from tests.abi_emulator import _fsm, _logitedit
from tests.test_ragged import SAMPLED, V, _gen, _model, _prompts, _ragged

f32 = np.float32
INF = np.inf
NSLOT = 53
END = V - 1
PEN = dict(repetition_penalty=1.8, presence_penalty=0.7, frequency_penalty=0.4)


def _choices(n=16, seed=0, vocab=V, end=END):
    """n distinct token sequences of 1 .. 3 tokens (some a proper prefix of another), none holding `end`."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        q = rng.integers(0, vocab - 1, 1 + len(out) % 3).tolist()
        if end not in q and q not in out:
            out.append(q)
    out[1] = out[2][:1] if out[2][:1] not in out else out[1]     # (a proper prefix of another choice)
    return out


CHOICES = _choices()
CHOICE = TokenFSM.from_sequences(CHOICES, END)
FREE = TokenFSM.free_until(7, TokenFSM.from_sequences([[1, 2], [3]], 0))


def _walk(fsm, toks):
    """A plain-Python walk of `fsm` over `toks`: False at the first token its state does not allow."""
    s = fsm.start
    for t in toks:
        edges = {int(fsm.tokens[j]): int(fsm.next[j]) for j in range(int(fsm.offsets[s]), int(fsm.offsets[s + 1]))}
        if t in edges:
            s = edges[t]
        elif fsm.dflt[s] >= 0:
            s = int(fsm.dflt[s])
        else:
            return False
    return True


def _is_choice(toks, choices=CHOICES, end=END):
    """toks = one of the choices, then `end` for the rest (or a prefix of that, when the budget ran out)."""
    return any(list(toks) == (c + [end] * len(toks))[:len(toks)] for c in choices)


def _lp_steps(m, it):
    """A run with logprobs: [(tokens (B,), Logprobs of the step)]."""
    m.eval()
    try:
        with pdn.no_grad():
            return [(t.numpy().reshape(-1).copy(), lp) for t, lp in it]
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _serve_all(m, prompts, budgets, **kw):
    m.eval()
    try:
        with pdn.no_grad():
            return m.serve_all(prompts, budgets, **kw)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


# -- the machine ------------------------------------------------------------------------------------------------------
def test_csr_form_and_defaults():
    m = TokenFSM([{5: 1, 2: 0}, {9: 1}, {}], start=1, default=[-1, None, 0])
    assert m.S == 3 and m.E == 3 and m.start == 1
    assert m.offsets.tolist() == [0, 2, 3, 3] and m.tokens.tolist() == [2, 5, 9] and m.next.tolist() == [0, 1, 1]
    assert m.dflt.tolist() == [-1, -1, 0] and all(a.dtype == np.int32 for a in m.arrays())
    assert F.MAX_STATES == 65536 and F.MAX_EDGES == 1 << 22


BAD = [dict(transitions=[{-1: 0}]), dict(transitions=[{1: 1}]), dict(transitions=[{1: -1}]),     # ids / states outside
       dict(transitions=[{1.5: 0}]), dict(transitions=[{1: 0.0}]), dict(transitions=[{"1": 0}]),
       dict(transitions=[{True: 0}]), dict(transitions=[{1: 0}], start=1.0),                     # non-integers
       dict(transitions=[{1: 0}, {}]), dict(transitions=[{1: 0}, {}], default=[0, -1]),           # nothing to pick
       dict(transitions=[]), dict(transitions={1: 0}), dict(transitions=[[1, 0]]),
       dict(transitions=[{1: 0}], start=1), dict(transitions=[{1: 0}], start=-1),
       dict(transitions=[{1: 0}], default=[1]), dict(transitions=[{1: 0}], default=[-2]),
       dict(transitions=[{1: 0}], default=[0, 0]), dict(transitions=[{1: 0}], default=[0.5])]


@pytest.mark.parametrize("bad", BAD)
def test_bad_machines_raise(bad):
    with pytest.raises(ValueError):
        TokenFSM(**bad)


def test_caps_raise(monkeypatch):
    monkeypatch.setattr(F, "MAX_STATES", 4)
    with pytest.raises(ValueError, match="MAX_STATES"):
        TokenFSM([{1: 0}] * 5)
    a, b = TokenFSM([{1: 0}] * 3), TokenFSM([{2: 0}] * 3)
    with pytest.raises(ValueError, match="MAX_STATES"):
        F.check_args([a, b], 10, 2)                              # (each fits, together they do not)
    assert F.check_args([a, a], 10, 2).tables.S == 3              # (one machine, merged once)
    monkeypatch.setattr(F, "MAX_STATES", 65536)
    monkeypatch.setattr(F, "MAX_EDGES", 3)
    with pytest.raises(ValueError, match="MAX_EDGES"):
        TokenFSM([{1: 0, 2: 0}, {1: 0, 2: 0}])
    with pytest.raises(ValueError, match="MAX_EDGES"):
        F.check_args([a, b], 10, 2)


def test_check_args():
    m = TokenFSM([{3: 0}])
    assert F.check_args(None, 10, 3) is None and F.check_args([None, None], 10, 2) is None
    assert F.check_args(None, 10, 3, speculate=4) is None
    spec = F.check_args(m, 10, 3)
    assert spec.starts.tolist() == [0, 0, 0] and spec.tables.S == 1
    other = TokenFSM([{1: 1}, {2: 0}], start=1)
    spec = F.check_args([m, None, other, m], 10, 4)
    assert spec.starts.tolist() == [0, -1, 2, 0] and spec.tables.S == 3
    assert spec.start_states([2, -1, 1, 0]).tolist() == [2, -1, -1, 0]
    assert spec.caps[0] >= 3 and spec.caps[1] >= 3 and all(c & (c - 1) == 0 for c in spec.caps)
    for bad in (dict(token_fsm=[m]), dict(token_fsm=[m, m, m]), dict(token_fsm="abc"), dict(token_fsm=3),
                dict(token_fsm=[m, {3: 0}]), dict(token_fsm={0: m}), dict(token_fsm=TokenFSM([{10: 0}])),
                dict(token_fsm=[None, TokenFSM([{1: 0, 11: 0}])]), dict(token_fsm=m, speculate=2)):
        with pytest.raises(ValueError):
            F.check_args(V=10, n=2, **bad)


def test_from_sequences_against_enumeration():
    """Every token sequence of length <= 4 over a vocabulary of 5: accepted exactly when it is a prefix of some choice
    followed by ends."""
    seqs, end = [[0, 1], [0], [2, 2, 1], [3]], 4
    m = TokenFSM.from_sequences(seqs, end)
    assert m.dflt.max() == -1
    for n in range(1, 5):
        for toks in itertools.product(range(5), repeat=n):
            assert _walk(m, toks) == _is_choice(toks, seqs, end), toks
    # the allowed continuations, state by state: after [0] both the end and the continuation
    z = np.zeros((3, 5), f32)
    s0 = F.advance(m, [m.start] * 3, [0, 2, 3])
    got = F.apply(z, m, s0)
    assert got[0].tolist() == [-INF, 0, -INF, -INF, 0] and got[1].tolist() == [-INF, -INF, 0, -INF, -INF]
    assert got[2].tolist() == [-INF, -INF, -INF, -INF, 0]
    term = F.advance(m, s0[2:], [end])
    assert F.advance(m, term, [end]).tolist() == term.tolist() and F.apply(z[:1], m, term)[0].tolist() == got[2].tolist()
    for bad in ([], [[]], [[1], []], [[1, 2], [1, 2]], [[1, end]], [[1.5]]):
        with pytest.raises(ValueError):
            TokenFSM.from_sequences(bad, end)
    with pytest.raises(ValueError):
        TokenFSM.from_sequences([[1]], 2.0)


def test_free_until():
    then = TokenFSM.from_sequences([[1, 2], [3]], 0)
    m = TokenFSM.free_until(7, then)
    assert m.S == then.S + 1 and m.dflt[0] == 0 and (m.dflt[1:] == -1).all() and m.start == 0
    assert _walk(m, [5, 9, 1, 7, 3, 0, 0]) and _walk(m, [7, 1, 2, 0]) and not _walk(m, [4, 7, 2]) and not _walk(m, [7, 7])
    z = np.arange(10, dtype=f32)[None]
    assert np.array_equal(F.apply(z, m, [0]), z)                 # a default state masks nothing
    assert F.advance(m, [0, 0], [4, 7]).tolist() == [0, then.start + 1]
    with pytest.raises(ValueError):
        TokenFSM.free_until(7, [{1: 0}])
    with pytest.raises(ValueError):
        TokenFSM.free_until("7", then)


def test_apply_and_advance_on_arrays():
    m = TokenFSM([{1: 1, 3: 0}, {0: 1}, {2: 0}], default=[-1, -1, 1])
    z = np.array([[1, 2, np.nan, 4], [1, 2, 3, 4], [1, 2, 3, 4], [INF, 2, 3, 4], [1, 2, 3, 4]], f32)
    got = F.apply(z, m, [0, 1, 2, -1, 7])
    assert got[0].tolist() == [-INF, 2, -INF, 4] and got[1].tolist() == [1, -INF, -INF, -INF]    # (a banned NaN: -inf)
    assert got[2].tolist() == [1, 2, 3, 4] and got[3].tolist() == [INF, 2, 3, 4] and got[4].tolist() == [1, 2, 3, 4]
    assert got.dtype == np.float32 and np.isnan(z[0, 2])          # (a new array)
    # explicit edge, default, the default's override, off, a state outside the tables
    assert F.advance(m, [0, 2, 2, -1, 7], [3, 0, 2, 1, 1]).tolist() == [0, 1, 0, -1, 7]


def test_missing_transition_keeps_the_state():
    """A token with neither an edge nor a default -- possible only when other edits banned everything the machine allows
    -- keeps the state: deterministic, on arrays, in the host rows and on the emulated plan alike."""
    m = TokenFSM([{1: 1}, {2: 0}])
    assert F.advance(m, [0, 1, 0], [2, 1, -1]).tolist() == [0, 1, 0]
    spec = F.check_args(m, 4, 2)
    rows = F.Rows(2, spec, [0, 1], [3, 3])
    z = np.zeros((2, 4), f32)
    assert rows.step(z, [9, 9], [3, 3]).tolist() == [[-INF, 0, -INF, -INF]] * 2                  # g = 0: the start state
    got = rows.step(z, [1, 3], [4, 4])                           # row 0 fed 1 -> state 1; row 1 fed 3: kept in state 0
    assert got.tolist() == [[-INF, -INF, 0, -INF], [-INF, 0, -INF, -INF]]
    assert F.unpair(rows.word)[0].tolist() == [1, 0] and F.unpair(rows.word)[1].tolist() == [4, 4]
    again = rows.step(z, [2, 2], [4, 4])                         # the same position again: the word is taken as it is
    assert np.array_equal(again, got) and F.unpair(rows.word)[0].tolist() == [1, 0]
    got = rows.step(z, [2, 1], [5, -1])                          # row 1 computes nothing: untouched, its word kept
    assert got.tolist() == [[-INF, 0, -INF, -INF], [0, 0, 0, 0]] and F.unpair(rows.word)[1].tolist() == [5, 4]


def test_packed_and_its_inverse():
    a = TokenFSM([{5: 1, 2: 0}, {9: 1}, {}], start=1, default=[-1, -1, 0])
    t, starts = F.packed([CHOICE, None, a, CHOICE, FREE])
    assert starts.tolist() == [0, -1, CHOICE.S + 1, 0, CHOICE.S + a.S] and t.S == CHOICE.S + a.S + FREE.S
    assert t.E == CHOICE.E + a.E + FREE.E and t.offsets[-1] == t.E and (np.diff(t.offsets) >= 0).all()
    for s in range(t.S):
        assert (np.diff(t.tokens[t.offsets[s]:t.offsets[s + 1]]) > 0).all()      # sorted within each state
    back = F.unpacked(t, starts[2])
    toks = [[9, 9, 9], [9, 5], [5], [2, 2, 9]]
    assert [_walk(back, q) for q in toks] == [_walk(a, q) for q in toks] == [True, False, False, False]
    one, s1 = F.packed([a])
    rt = F.unpacked(one, s1[0])
    assert all(np.array_equal(x, y) for x, y in zip(rt.arrays(), a.arrays())) and rt.start == a.start
    off, tok, nxt, dfl = F.padded(one, 8, 16)
    assert off.tolist() == [0, 2, 3, 3, 3, 3, 3, 3, 3] and tok.shape == nxt.shape == (16,) and dfl.tolist()[3:] == [-1] * 5
    with pytest.raises(ValueError):
        F.padded(one, 2, 16)
    assert F.unpair(F.pair([3, -1], [7, 0]))[0].tolist() == [3, -1] and F.unpair(F.pair([3, -1], [7, 0]))[1].tolist() == [7, 0]


# -- the public interface ---------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(emulated_hip):
    from pydynet_amd import _lib
    _fsm.extend()
    m = _model("hip:0")
    prompts = _prompts([2, 3])
    n0 = len(_lib._LIB.calls)
    for bad in (dict(token_fsm=TokenFSM([{V: 0}])), dict(token_fsm=[CHOICE]), dict(token_fsm="x"),
                dict(token_fsm=[CHOICE, 3])):
        for call in (lambda: m.generate(np.stack(_prompts([3, 3])), 8, **bad), lambda: m.generate_ragged(prompts, 4, **bad),
                     lambda: m.serve(prompts, 4, **bad), lambda: m.serve(prompts, 4, prefill_chunk=2, **bad),
                     lambda: m.serve_all(prompts, 4, **bad)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="speculate"):
        m.generate_ragged(prompts, 4, speculate=2, token_fsm=CHOICE)
    m.generate_ragged(prompts, 4, speculate=2, token_fsm=None)
    assert len(_lib._LIB.calls) == n0
    with pytest.raises(TypeError):
        m.beam_search(prompts, 4, 2, token_fsm=CHOICE)           # (out of scope)


def _machines(N):
    """Per request: the 16-way choice, the free-until machine, none, the choice again."""
    return [(CHOICE, FREE, None, CHOICE)[r % 4] for r in range(N)]


def _check_rows(rows, fsms):
    for r, (toks, f) in enumerate(zip(rows, fsms)):
        toks = [int(t) for t in toks if t >= 0]
        if f is not None:
            assert _walk(f, toks), (r, toks)
        if f is CHOICE:
            assert _is_choice(toks), (r, toks)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (2, SAMPLED[2]), (12, {})])
def test_emulated_generate_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    _fsm.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    ids = np.stack(_prompts([5] * B, seed=13))
    fsms = _machines(B)
    want = _gen(_model("cpu", B=max(B, 5)), ids, 5 + 10, **kw, token_fsm=fsms)
    counters(NSLOT)
    m = _model("hip:0", B=max(B, 5))
    got = _gen(m, ids, 5 + 10, **kw, token_fsm=fsms)
    # one reset for the run, one launch per decode step and one for the prompt pass
    assert np.array_equal(got, want) and counters(NSLOT)[52] == 11 and m._decode_st["fsm"] and m._decode_st["full"]
    assert not np.array_equal(got, _gen(_model("cpu", B=max(B, 5)), ids, 5 + 10, **kw))
    _check_rows(got, fsms)
    # one machine for the whole call, a second generation on the same plan
    want = _gen(_model("cpu", B=max(B, 5)), ids, 5 + 6, **kw, token_fsm=CHOICE)
    got = _gen(m, ids, 5 + 6, **kw, token_fsm=CHOICE)
    assert np.array_equal(got, want)
    _check_rows(got, [CHOICE] * B)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (5, SAMPLED[1]), (12, {}), (10, SAMPLED[0])])
def test_emulated_generate_ragged_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    _fsm.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    prompts = _prompts([1 + (3 * i) % 7 for i in range(B)], seed=12)
    fsms = _machines(B)
    kw = dict(kw, stop_ids=[END], token_fsm=fsms)
    want = _ragged(_model("cpu", B=max(B, 5)), prompts, 9, **kw)
    m = _model("hip:0", B=max(B, 5))
    counters(NSLOT)
    got = _ragged(m, prompts, 9, **kw)
    c = counters(NSLOT)
    st = m._decode_st
    assert np.array_equal(got, want) and st["fsm"] and c[52] == got.shape[1] + 1 and c[48] == 0 and c[35] == 0
    assert st["fsm_start"].get().tolist() == [p.size for p in prompts]
    assert st["fsm_start_state"].get().tolist() == F.check_args(fsms, V, B).starts.tolist()
    _check_rows(got, fsms)
    for r in range(0, B, 4):                                     # a choice row: one of the choices, the end, then stopped
        toks = got[r].tolist()
        assert END in toks and all(t == -1 for t in toks[toks.index(END) + 1:]), toks


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("S,chunk,prefix,kw", [(3, None, False, {}), (3, 4, False, {}), (3, 4, True, {}),
                                                (2, None, False, SAMPLED[1]), (10, None, False, {}),
                                                (10, 3, True, SAMPLED[0])])
def test_emulated_serve_equals_cpu(emulated_hip, graphs, S, chunk, prefix, kw, monkeypatch):
    _fsm.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    N = S + 4
    rng = np.random.default_rng(14)
    head = rng.integers(0, V, 3)                                 # (a shared start: the prefix cache has something to reuse)
    prompts = [np.concatenate([head, rng.integers(0, V, 1 + (5 * i) % 6)]) for i in range(N)]
    budgets = [2 + (3 * i) % 7 for i in range(N)]
    fsms = _machines(N)
    kw = dict(kw, slots=S, stop_ids=[END], prefill_chunk=chunk, prefix_cache=prefix, token_fsm=fsms)
    want = _serve_all(_model("cpu", B=N), prompts, budgets, **kw)
    counters(NSLOT)
    m = _model("hip:0", B=N)
    got = _serve_all(m, prompts, budgets, **kw)
    assert [g.tolist() for g in got] == [w.tolist() for w in want] and counters(NSLOT)[52] > 0 and m._decode_st["fsm"]
    if prefix:
        assert m.prefix_stats["hits"] > 0
    _check_rows([g.tolist() for g in got], fsms)
    plain = _serve_all(_model("cpu", B=N), prompts, budgets, **dict(kw, token_fsm=None))
    assert [g.tolist() for g in got] != [p.tolist() for p in plain]
    for r in range(2, N, 4):                                     # a request without a machine: its plain tokens
        assert got[r].tolist() == plain[r].tolist()


def test_cpu_serve_all_equals_generate_ragged():
    """The serve promise holds with machines: request r's tokens are row r's of generate_ragged, whichever row it runs in."""
    prompts = _prompts([3, 1, 6, 2, 4, 5, 2], seed=8)
    budgets = [6, 3, 9, 1, 7, 4, 8]
    fsms = _machines(7)
    full = _ragged(_model("cpu", B=7), prompts, 9, token_fsm=fsms)
    _check_rows(full, fsms)
    for chunk in (None, 3):
        got = _serve_all(_model("cpu", B=7), prompts, budgets, slots=3, prefill_chunk=chunk, token_fsm=fsms)
        assert [g.tolist() for g in got] == [r[:b].tolist() for r, b in zip(full, budgets)]


def test_emulated_with_penalties_edits_and_logprobs(emulated_hip):
    """Penalties, the machine, edits and logprobs together, in that order: tokens and records as on `cpu`; a token the
    machine bans has log-probability -inf, and a bias cannot revive it."""
    _fsm.extend()
    _logitedit.extend()
    Graph.clear()
    two = TokenFSM([{11: 0, 40: 0}])
    for B in (4, 11):
        prompts = _prompts([1 + (3 * i) % 5 for i in range(B)], seed=31)
        fsms = _machines(B)
        fsms[1] = two
        bias = [None] * B
        bias[1], bias[2] = {5: 1e30, 11: -1.0}, {3: 2.0}
        kw = dict(logprobs=3, token_fsm=fsms, logit_bias=bias, **PEN)
        mc, mh = _model("cpu", B=B), _model("hip:0", B=B)
        want = _lp_steps(mc, mc.generate_ragged(prompts, 8, **kw))
        counters(NSLOT)
        got = _lp_steps(mh, mh.generate_ragged(prompts, 8, **kw))
        c = counters(NSLOT)
        st = mh._decode_st
        assert c[52] == 9 and c[48] == 9 and c[35] == 9 and st["fsm"] and st["edit"] and st["pen"]
        for (gt, gl), (wt, wl) in zip(got, want):
            assert np.array_equal(gt, wt) and np.array_equal(gl.top_ids, wl.top_ids)
            assert np.allclose(gl.token, wl.token, rtol=1e-5, atol=1e-4, equal_nan=True)
            assert gt[1] in (11, 40) and gl.top_logprobs[1, 2] == -INF and np.isfinite(gl.top_logprobs[1, :2]).all()
        _check_rows(np.stack([g[0] for g in got], 1), fsms)


def test_emulated_refusing_library_follows_the_statement(emulated_hip, monkeypatch):
    """Without the pdnf_ entries (the emulator not extended) every path applies the statement on the host; and with the
    step entry removed the plan refuses likewise.  Tokens as on `cpu`."""
    from pydynet_amd import _lib
    prompts = _prompts([3, 6, 2], seed=15)
    fsms = _machines(3)
    want = _ragged(_model("cpu"), prompts, 9, token_fsm=fsms)
    budgets = [5, 7, 3]
    served = [w.tolist() for w in _serve_all(_model("cpu"), prompts, budgets, slots=2, token_fsm=fsms)]
    for extended in (False, True):
        Graph.clear()
        if extended:
            _fsm.extend()
            remove(monkeypatch, _lib._LIB, "pdnf_fsm_step_f32")
        assert not _lib.provides("pdnf_fsm_step_f32")
        counters(NSLOT)
        m = _model("hip:0")
        got = _ragged(m, prompts, 9, token_fsm=fsms)
        c = counters(NSLOT)
        assert np.array_equal(got, want) and c[52] == 0 and c[29] > 0 and m._decode_st["ok"] is False
        assert [g.tolist() for g in _serve_all(_model("hip:0"), prompts, budgets, slots=2, token_fsm=fsms)] == served


def test_default_launches_unchanged(emulated_hip):
    """With token_fsm=None the plan key, the launches and the counters are those of a run without the keyword."""
    from pydynet_amd import _lib
    _fsm.extend()
    Graph.clear()
    ids = np.stack(_prompts([4, 4], seed=10))
    runtime = ("pdn_malloc", "pdn_free", "pdn_set_device", "pdn_compute_stream", "pdn_fill", "pdn_kernel_counters",
               "pdn_memcpy")                                   # (allocator / setup traffic differs between first uses)

    def run(fn):
        _lib._LIB.calls.clear()
        counters(NSLOT)
        out = fn()
        return out, counters(NSLOT), [c for c in _lib._LIB.calls if not c.startswith(runtime)]
    m0, m1 = _model("hip:0"), _model("hip:0")
    base, c0, calls0 = run(lambda: _gen(m0, ids, 14))
    again, c1, calls1 = run(lambda: _gen(m1, ids, 14, token_fsm=None))
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[52] == 0
    assert not any("fsm" in c for c in calls0)
    k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
    assert len(k0) == len(k1) and "fsm" not in k1 and m1._decode_st["fsm"] is False and "fsm_off" not in m1._decode_st
    prompts = _prompts([3, 5, 2], seed=11)
    m0, m1 = _model("hip:0"), _model("hip:0")
    base, c0, calls0 = run(lambda: _ragged(m0, prompts, 6, stop_ids=[5]))
    again, c1, calls1 = run(lambda: _ragged(m1, prompts, 6, stop_ids=[5], token_fsm=[None] * 3))
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[52] == 0
    assert len(m0._decode_st["key"]) == len(m1._decode_st["key"]) == len(k0)
    base, c0, calls0 = run(lambda: [o.tolist() for o in _serve_all(m0, prompts, 5, slots=2, prefill_chunk=2)])
    again, c1, calls1 = run(lambda: [o.tolist() for o in _serve_all(m1, prompts, 5, slots=2, prefill_chunk=2,
                                                                     token_fsm=None)])
    assert base == again and c0 == c1 and calls0 == calls1 and c0[52] == 0
    # with a machine the key grows by the term and the capacity; a machine of similar size keeps the plan
    _ragged(m1, prompts, 6, token_fsm=CHOICE)
    key = m1._decode_st["key"]
    assert key[-3] == "fsm" and len(key) == len(k0) + 3 and key[-2:] == F.check_args(CHOICE, V, 3).caps
    _ragged(m1, prompts, 6, token_fsm=FREE)
    assert m1._decode_st["key"] == key


def test_emulated_entries_follow_the_statement(emulated_hip):
    """The emulated reset / step / rows entries through the library's call path: the statement on random rows."""
    from pydynet_amd import _lib, hipnp as hp
    _fsm.extend()
    rng = np.random.default_rng(16)
    B, Vv = 5, 2500
    edges = TokenFSM([{0: 1, 1023: 1, 1024: 2, 1475: 0, 1476: 0, 2499: 1}, {7: 0}, {}, {5: 3, 9: 0}], default=[-1, -1, 2, 1])
    spec = F.check_args([edges, None, edges, edges, edges], Vv, B)
    S_cap, E_cap = spec.caps
    tabs = [hp.asarray(a) for a in F.padded(spec.tables, S_cap, E_cap)]
    L = _lib.lib()
    n = L.query("pdnf_fsm_chunks", Vv)
    assert n == 3 and L.query("pdnf_fsm_chunks", 0) == 0 and L.query("pdnf_fsm_chunks", 1024) == 1
    z = (5 * rng.standard_normal((B, Vv))).astype(f32)
    # the reset into a zeroed state, rows permuted, one row outside
    st = [hp.zeros((B,), np.int64), hp.zeros((B,), np.int32), hp.zeros((B,), np.int32)]
    states, start = np.array([0, -1, 1, 3, 0], np.int32), np.array([3, 1, 5, 2, 4], np.int32)
    order, pick = np.array([2, 0, 9, 3, 1, 4], np.int32), np.array([2, 0, 0, 3, 1, 4])
    src = [hp.asarray(np.ascontiguousarray(a)) for a in (order, states[pick], start[pick])]
    L.call("pdnf_fsm_reset", *(a._ptr for a in st), B, src[0]._ptr, 6, src[1]._ptr, src[2]._ptr, hp.stream())
    assert np.array_equal(st[0].get(), F.pair(states, start)) and np.array_equal(st[1].get(), states)
    assert np.array_equal(st[2].get(), start)
    # row 0: g = 1, fed 1024 -> state 2 (a default: no mask); row 1: off; row 2: stopped; row 3: g = 0 -> state 3 (a default
    # with overrides: no mask); row 4: g = 2 with a stale word: fed 7 in state 0, no edge, no default -> kept
    pos, ids = np.array([4, 9, -1, 2, 6], np.int32), np.array([1024, 3, 7, 5, 7], np.int64)
    want = z.copy()
    want[4] = F.apply(z[4:], edges, [0])[0]
    x, P, I = hp.asarray(z), hp.asarray(pos), hp.asarray(ids.reshape(B, 1))
    cv, ci = hp.asarray(np.full((B, n), 7.0, f32)), hp.asarray(np.full((B, n), -7, np.int32))
    L.call("pdnf_fsm_step_f32", x._ptr, Vv, B, Vv, *(a._ptr for a in tabs), S_cap, E_cap, *(a._ptr for a in st), I._ptr,
           P._ptr, 1, cv._ptr, ci._ptr, hp.stream())
    assert np.array_equal(x.get().view(np.int32), want.view(np.int32))
    assert np.isfinite(want[4, [0, 1023, 1024, 1475, 1476, 2499]]).all() and np.isinf(want[4]).sum() == Vv - 6
    assert F.unpair(st[0].get())[0].tolist() == [2, -1, 1, 3, 0] and F.unpair(st[0].get())[1].tolist() == [4, 9, 5, 2, 6]
    assert ci.get()[4].tolist() == [int(np.argmax(want[4, :1024])), 1024 + int(np.argmax(want[4, 1024:2048])),
                                    2048 + int(np.argmax(want[4, 2048:]))]
    assert (cv.get()[2] == 7.0).all() and (ci.get()[2] == -7).all() and cv.get()[0, 0] == want[0, :1024].max()
    # the next step: row 0 leaves its default state by the default (fed 8 -> 2), row 3 by an override (fed 9 -> 0)
    I, P = hp.asarray(np.array([8, 3, 7, 9, 2499], np.int64).reshape(B, 1)), hp.asarray(pos + (pos >= 0))
    L.call("pdnf_fsm_step_f32", x._ptr, Vv, B, Vv, *(a._ptr for a in tabs), S_cap, E_cap, *(a._ptr for a in st), I._ptr,
           P._ptr, 1, None, None, hp.stream())
    assert F.unpair(st[0].get())[0].tolist() == [2, -1, 1, 0, 1]
    # (row 4, now in state 1, keeps token 7 alone -- which its first step had banned already: nothing is left)
    assert np.isinf(x.get()[3]).sum() == Vv - 6 and np.isinf(x.get()[4]).all() and np.array_equal(x.get()[0], z[0])
    # the rows form: explicit states, read only
    x = hp.asarray(z)
    d = hp.asarray(np.array([1, -1, 0, 2, 3], np.int32))
    P = hp.asarray(np.array([0, 0, -1, 0, 0], np.int32))
    L.call("pdnf_fsm_rows_f32", x._ptr, Vv, B, Vv, tabs[0]._ptr, tabs[1]._ptr, tabs[3]._ptr, S_cap, E_cap, d._ptr,
           P._ptr, None, None, hp.stream())
    want = F.apply(z, edges, [1, -1, -1, 2, 3])
    assert np.array_equal(x.get().view(np.int32), want.view(np.int32)) and np.isinf(want[0]).sum() == Vv - 1
    assert d.get().tolist() == [1, -1, 0, 2, 3]
    for a, b in zip(tabs, F.padded(spec.tables, S_cap, E_cap)):
        assert np.array_equal(a.get(), b)                        # the tables are only read
