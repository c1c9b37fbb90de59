"""Repetition, presence and frequency penalties (`generate`, `generate_ragged`, `serve`, `serve_all`) on the CPU: the
statement of llm/penalties.py by hand cases, the `cpu` device against a hand loop of `forward_logits` plus the statement,
`serve_all` against `generate_ragged`, argument errors, and the emulated C ABI with the entry points of
tests/abi_emulator/_penalty.py (the graph-replayed steps, with and without graphs) against `cpu`."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core import Tensor
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import penalties, sampling
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import apply_np, counters, remove, reset_np
from tests.test_ragged import SAMPLED, V, _gen, _model, _prompts, _ragged

PEN = dict(repetition_penalty=1.8, presence_penalty=0.7, frequency_penalty=0.4)
PENS = [PEN, dict(repetition_penalty=1.3), dict(presence_penalty=1.5, frequency_penalty=0.25)]


def _values(kw):
    return penalties.check_args(**kw)


def _f32(x):
    return np.float32(x)


# -- the statement ----------------------------------------------------------------------------------------------------
def test_repetition_acts_once_for_a_token_generated_three_times():
    z = np.array([[2.0, -1.0, 3.0, 0.5]], np.float32)
    c = np.array([[0, 3, 1, 0]])
    got = penalties.penalize(z, c, np.zeros((1, 4), bool), 2.0, 0.0, 0.0)
    assert got.tolist() == [[2.0, -2.0, 1.5, 0.5]]


def test_presence_and_frequency_ignore_prompt_only_tokens():
    z = np.array([[3.0, 3.0, 3.0]], np.float32)
    seen = np.array([[True, False, True]])
    c = np.array([[0, 0, 2]])
    got = penalties.penalize(z, c, seen, 1.0, 0.5, 0.25)
    assert got.tolist() == [[3.0, 3.0, 2.0]]                  # token 0: prompt only; token 2: 3 - (0.25 * 2 + 0.5)
    got = penalties.penalize(z, c, seen, 2.0, 0.5, 0.25)
    assert got.tolist() == [[1.5, 3.0, 0.5]]                  # repetition acts on the prompt token, then 1.5 - 1.0


def test_negative_logit_is_multiplied():
    z = np.array([[-1.5, 1.5, 0.0, -0.0]], np.float32)
    got = penalties.penalize(z, np.zeros((1, 4), np.int64), np.ones((1, 4), bool), 1.3, 0.0, 0.0)
    assert got[0, 0] == _f32(-1.5) * _f32(1.3) and got[0, 1] == _f32(1.5) / _f32(1.3)
    assert got[0, 2] == 0.0 and np.signbit(got[0, 3])           # zeros are multiplied: the sign stays


def test_infinities_stay():
    z = np.array([[-np.inf, np.inf, -np.inf, 1.0]], np.float32)
    c = np.array([[1, 2, 0, 0]])
    got = penalties.penalize(z, c, np.array([[False, False, True, False]]), 1.7, 0.3, 0.9)
    assert got[0, 0] == -np.inf and got[0, 1] == np.inf and got[0, 2] == -np.inf and got[0, 3] == 1.0


def test_float32_order_of_operations():
    rng = np.random.default_rng(0)
    z = rng.standard_normal((3, 50)).astype(np.float32) * 7
    c = rng.integers(0, 4, (3, 50))
    seen = rng.random((3, 50)) < 0.3
    r, p, f = 1.37, 0.61, 0.173
    got = penalties.penalize(z, c, seen, r, p, f)
    want = z.copy()
    for b in range(3):
        for v in range(50):
            x = z[b, v]
            if seen[b, v] or c[b, v] > 0:
                x = x / _f32(r) if x > 0 else x * _f32(r)
            if c[b, v] > 0:
                x = x - (_f32(f) * _f32(c[b, v]) + _f32(p))
            want[b, v] = x
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_defaults_are_off():
    assert penalties.check_args() is None
    assert penalties.check_args(1, 0, 0, speculate=4) is None
    assert penalties.check_args(1.5) == (1.5, 0.0, 0.0)


# -- the `cpu` device against a hand loop -------------------------------------------------------------------------------
def _hand(prompts, n, pen, kw=None, stops=()):
    """Row by row on a fresh model: forward_logits over the prompt, then one token per call at the positions `generate`
    feeds it (step i >= 1 at len + i), the statement, the pick / draw."""
    kw = kw or {}
    out = []
    try:
        with pdn.no_grad():
            for b, q in enumerate(prompts):
                m = _model("cpu", B=1)
                m.eval()
                seq, toks = [int(t) for t in q], []
                for i in range(n):
                    feed, at = (seq, 0) if i == 0 else (seq[-1:], len(q) + i)
                    z = np.asarray(m.forward_logits(Tensor(np.array([feed], np.int64), dtype=np.int64), at).numpy(),
                                   np.float32)[0, -1]
                    c = np.bincount(np.array(toks, np.int64), minlength=V)
                    z = penalties.penalize(z[None], c[None], penalties.seen_rows([q], V), *pen)
                    if kw.get("temperature", 0) > 0:
                        t = int(sampling.sample_rows_np(z, len(seq), kw["temperature"], kw.get("top_k", 0),
                                                        kw.get("top_p", 1.0), kw.get("seed", 0), rows=[b])[0])
                    else:
                        t = int(np.argmax(z[0]))
                    toks.append(t)
                    seq.append(t)
                    if t in stops:
                        break
                out.append(toks)
    finally:
        pdn.autograd.set_grad_enabled(True)
    return out


def _rows(a):
    """generate_ragged's (B, steps) array -> each row's tokens (up to its first -1)."""
    return [[int(t) for t in r[:np.argmax(r < 0)] if t >= 0] if (r < 0).any() else [int(t) for t in r] for r in a]


@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
@pytest.mark.parametrize("pen", PENS)
def test_cpu_generate_ragged_equals_hand_loop(kw, pen):
    prompts = _prompts([3, 1, 6, 2], seed=4)
    got = _ragged(_model("cpu"), prompts, 10, **kw, **pen)
    assert _rows(got) == _hand(prompts, 10, _values(pen), kw)
    assert not np.array_equal(got, _ragged(_model("cpu"), prompts, 10, **kw))    # the penalties change the tokens


@pytest.mark.parametrize("kw", [{}, SAMPLED[0]])
def test_cpu_generate_equals_hand_loop(kw):
    ids = np.stack(_prompts([4, 4, 4], seed=5))
    got = _gen(_model("cpu"), ids, 4 + 9, **kw, **PEN)
    assert [list(r) for r in got.tolist()] == _hand(list(ids), 9, _values(PEN), kw)


def test_cpu_stop_ids_with_penalties():
    prompts = _prompts([2, 5, 3], seed=6)
    free = _ragged(_model("cpu"), prompts, 12, **PEN)
    stops = sorted({int(free[0, 4]), int(free[1, 2])})
    got = _ragged(_model("cpu"), prompts, 12, stop_ids=stops, **PEN)
    assert _rows(got) == _hand(prompts, 12, _values(PEN), stops=stops)
    assert (got == -1).any()


def test_cpu_huge_presence_never_repeats():
    prompts = _prompts([3, 2, 4], seed=7)
    got = _ragged(_model("cpu"), prompts, 20, presence_penalty=1e4)
    for r in got:
        assert len(set(r.tolist())) == r.size


def _serve_all(m, prompts, budgets, **kw):
    m.eval()
    try:
        with pdn.no_grad():
            return [o.tolist() for o in m.serve_all(prompts, budgets, **kw)]
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _expected_serve(prompts, budgets, stops=(), **kw):
    """Request r: row r of generate_ragged(prompts, max(budgets), ...), cut at its budget (the serve promise)."""
    full = _ragged(_model("cpu", B=len(prompts)), prompts, int(max(budgets)), stop_ids=stops, **kw)
    return [r[:b] for r, b in zip(_rows(full), budgets)]


@pytest.mark.parametrize("chunk", [None, 3])
@pytest.mark.parametrize("kw", [{}, SAMPLED[2]])
def test_cpu_serve_all_equals_generate_ragged(kw, chunk):
    prompts = _prompts([3, 1, 6, 2, 4, 5, 2], seed=8)
    budgets = [6, 3, 9, 1, 7, 4, 8]
    want = _expected_serve(prompts, budgets, **kw, **PEN)
    got = _serve_all(_model("cpu", B=7), prompts, budgets, slots=3, prefill_chunk=chunk, **kw, **PEN)
    assert got == want


def test_cpu_serve_stop_ids_with_penalties():
    prompts = _prompts([2, 4, 3, 5, 1], seed=9)
    budgets = [8, 8, 8, 8, 8]
    free = _expected_serve(prompts, budgets, **PEN)
    stops = sorted({free[0][3], free[2][2]})
    want = _expected_serve(prompts, budgets, stops=stops, **PEN)
    for chunk in (None, 2):
        assert _serve_all(_model("cpu", B=5), prompts, budgets, slots=2, stop_ids=stops, prefill_chunk=chunk,
                          **PEN) == want


# -- arguments --------------------------------------------------------------------------------------------------------
BAD = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
       dict(repetition_penalty=float("inf")), dict(repetition_penalty=1e-60), dict(presence_penalty=float("inf")),
       dict(presence_penalty=float("nan")), dict(frequency_penalty=-float("inf")), dict(frequency_penalty=1e39),
       dict(presence_penalty="1"), dict(repetition_penalty=True), dict(frequency_penalty=None)]


@pytest.mark.parametrize("bad", BAD)
def test_bad_arguments_raise_before_any_launch(emulated_hip, bad):
    from pydynet_amd import _lib
    m = _model("hip:0")
    prompts = _prompts([2, 3])
    n0 = len(_lib._LIB.calls)
    for call in (lambda: m.generate(np.stack(_prompts([3, 3])), 8, **bad),
                 lambda: m.generate_ragged(prompts, 4, **bad),
                 lambda: m.serve(prompts, 4, **bad),
                 lambda: m.serve(prompts, 4, prefill_chunk=2, **bad),
                 lambda: m.serve_all(prompts, 4, **bad)):
        with pytest.raises(ValueError):
            call()
    assert len(_lib._LIB.calls) == n0


def test_penalties_refused_with_speculation():
    m = _model("cpu")
    with pytest.raises(ValueError, match="speculate"):
        m.generate_ragged(_prompts([2, 3]), 4, speculate=2, repetition_penalty=1.2)
    m.generate_ragged(_prompts([2, 3]), 4, speculate=2, repetition_penalty=1.0)      # (defaults: off)


# -- the emulated HIP path --------------------------------------------------------------------------------------------
def test_default_launches_unchanged(emulated_hip):
    from pydynet_amd import _lib
    Graph.clear()
    ids = np.stack(_prompts([4, 4], seed=10))
    _lib._LIB.calls.clear()
    counters()
    base = _gen(_model("hip:0"), ids, 14)
    c0, calls0 = counters(), list(_lib._LIB.calls)
    _lib._LIB.calls.clear()
    again = _gen(_model("hip:0"), ids, 14, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0)
    c1, calls1 = counters(), list(_lib._LIB.calls)
    runtime = ("pdn_malloc", "pdn_free", "pdn_set_device", "pdn_compute_stream", "pdn_fill", "pdn_kernel_counters",
               "pdn_memcpy")                                   # (allocator / setup traffic differs between first uses)
    calls0, calls1 = ([c for c in cl if not c.startswith(runtime)] for cl in (calls0, calls1))
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[35] == 0
    assert not any("penalty" in c for c in calls0)
    m = _model("hip:0")
    _ragged(m, _prompts([3, 5, 2], seed=11), 6)
    assert m._decode_st["pen"] is False and "counts" not in m._decode_st


def _fed_counts(got, prompts, n_rows, V):
    """bincount of the tokens each row was FED at a decode step: every yielded token but the row's last."""
    c = np.zeros((n_rows, V), np.int64)
    for b, r in enumerate(_rows(got)):
        np.add.at(c[b], np.array(r[:-1], np.int64), 1)
    return c


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (5, SAMPLED[1]), (12, {}), (10, SAMPLED[0])])
def test_emulated_generate_ragged_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    prompts = _prompts([1 + (3 * i) % 7 for i in range(B)], seed=12)
    want = _ragged(_model("cpu", B=max(B, 5)), prompts, 9, stop_ids=[5], **kw, **PEN)
    m = _model("hip:0", B=max(B, 5))
    counters()
    got = _ragged(m, prompts, 9, stop_ids=[5], **kw, **PEN)
    c = counters()
    assert np.array_equal(got, want)
    assert c[35] > 0 and m._decode_st["pen"]
    # the plan's counts: the tokens fed to its steps, nothing from the capture's runs
    assert np.array_equal(m._decode_st["counts"].get(), _fed_counts(got, prompts, B, V))


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (2, SAMPLED[2]), (12, {})])
def test_emulated_generate_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    ids = np.stack(_prompts([5] * B, seed=13))
    want = _gen(_model("cpu", B=max(B, 5)), ids, 5 + 10, **kw, **PEN)
    counters()
    got = _gen(_model("hip:0", B=max(B, 5)), ids, 5 + 10, **kw, **PEN)
    assert np.array_equal(got, want) and counters()[35] > 0


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("S,chunk,kw", [(3, None, {}), (3, 4, {}), (2, None, SAMPLED[1]), (10, None, {}),
                                         (10, 3, SAMPLED[0])])
def test_emulated_serve_equals_cpu(emulated_hip, graphs, S, chunk, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    N = S + 4
    prompts = _prompts([1 + (5 * i) % 6 for i in range(N)], seed=14)
    budgets = [2 + (3 * i) % 7 for i in range(N)]
    want = _serve_all(_model("cpu", B=N), prompts, budgets, slots=S, stop_ids=[7], prefill_chunk=chunk, **kw, **PEN)
    counters()
    got = _serve_all(_model("hip:0", B=N), prompts, budgets, slots=S, stop_ids=[7], prefill_chunk=chunk, **kw, **PEN)
    assert got == want and counters()[35] > 0


def test_emulated_refusing_library_follows_the_statement(emulated_hip, monkeypatch):
    """Without the penalty entries every path applies the statement on the host; tokens as on `cpu`."""
    from pydynet_amd import _lib
    Graph.clear()
    remove(monkeypatch, _lib._LIB, "pdn_penalty_step_f32")
    prompts = _prompts([3, 6, 2], seed=15)
    want = _ragged(_model("cpu"), prompts, 9, **PEN)
    counters()
    got = _ragged(_model("hip:0"), prompts, 9, **PEN)
    budgets = [5, 7, 3]
    served = _serve_all(_model("hip:0"), prompts, budgets, slots=2, **PEN)
    c = counters()
    assert np.array_equal(got, want) and c[35] == 0 and c[29] > 0
    assert served == _expected_serve(prompts, budgets, **PEN)


def test_emulated_entries_follow_the_statement(emulated_hip):
    """The emulated reset / apply entries through the library's call path: the statement on random rows."""
    from pydynet_amd import _lib, hipnp as hp
    rng = np.random.default_rng(16)
    B, Vv = 4, 2500
    z = rng.standard_normal((B, Vv)).astype(np.float32) * 5
    counts = rng.integers(0, 3, (B, Vv)).astype(np.int32)
    prompts = [rng.integers(0, Vv, n) for n in (3, 1, 7, 4)]
    seen = penalties.seen_bits(prompts, Vv)
    pos = np.array([4, -1, 9, 2], np.int32)
    want = z.copy()
    apply_np(want, (1.4, 0.3, 0.2), counts.astype(np.int64), seen, pos)
    x, prm, c, s, p = (hp.asarray(a) for a in (z, penalties.params_bytes(1.4, 0.3, 0.2), counts, seen, pos))
    _lib.lib().call("pdn_penalty_rows_f32", x._ptr, Vv, B, Vv, prm._ptr, c._ptr, s._ptr, p._ptr, None, None, hp.stream())
    assert np.array_equal(x.get().view(np.int32), want.view(np.int32))
    assert np.array_equal(x.get()[1], z[1])
    c, s, st = hp.asarray(counts), hp.zeros((B, -(-Vv // 32)), np.int32), hp.zeros((B,), np.int32)
    ids, off = penalties.packed(prompts[:2])
    rows, d_ids, d_off = hp.asarray(np.array([2, 0], np.int32)), hp.asarray(ids), hp.asarray(off)
    _lib.lib().call("pdn_penalty_reset", c._ptr, s._ptr, st._ptr, B, Vv, rows._ptr, 2, d_ids._ptr, d_off._ptr, hp.stream())
    wc, ws, wst = counts.astype(np.int32), np.zeros((B, -(-Vv // 32)), np.int32), np.zeros(B, np.int32)
    reset_np(wc, ws, wst, np.array([2, 0]), ids, off)
    assert np.array_equal(c.get(), wc) and np.array_equal(s.get(), ws) and wst.tolist() == [1, 0, 3, 0]
    assert np.array_equal(st.get(), wst)
