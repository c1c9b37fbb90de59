"""Chunked prefill (`Llama.serve(..., prefill_chunk=C)`) on the CPU: the schedule statement of llm/chunked.py by hand
cases, the `cpu` device against `serve`, and the emulated C ABI with the entry points of tests/abi_emulator/_extend.py
(the mixed step of the served plan, with and without graphs) against the `cpu` reference of tests/test_serve.py."""
import numpy as np
import pytest

from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import chunked
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters
from tests.test_serve import (BUDGETS, LENS, SAMPLED, _check, _eval, _model, _prompts, _reference, _serve_all, _stream,
                              _want)


def _drive(lens, budgets, S, C, tokens, stops=()):
    """Run the schedule with a token source tokens(req, position) -> token; returns the per-step (reqs, toks) and the
    per-step feeds (row -> (request, first position, count))."""
    sch = chunked.Schedule(lens, budgets, S, C)
    steps, feeds = [], []
    while True:
        sch.admit()
        if not sch.busy():
            return steps, feeds
        n, dec, comp = sch.plan()
        toks = np.full(S, -1, np.int64)
        for b in np.flatnonzero(dec | comp):
            p = sch.pos[b] if dec[b] else sch.row_lens()[b]
            toks[b] = tokens(int(sch.req[b]), int(p))
        feeds.append({int(b): (int(sch.req[b]), int(sch.fed[b]), int(n[b])) for b in np.flatnonzero(n)})
        shown = sch.finish(n, toks, stops)
        steps.append((shown.tolist(), toks.tolist()))


def _tok(r, p):
    return 100 * r + p


def test_schedule_prompt_over_several_steps():
    steps, feeds = _drive([7], [2], 1, 3, _tok)
    assert feeds == [{0: (0, 0, 3)}, {0: (0, 3, 3)}, {0: (0, 6, 1)}, {}]
    assert steps == [([0], [-1]), ([0], [-1]), ([0], [7]), ([0], [8])]


def test_schedule_two_rows_share_a_budget():
    steps, feeds = _drive([3, 4], [1, 1], 2, 5, _tok)
    # request 0 first (3 tokens), request 1 takes the 2 left, then its last 2
    assert feeds == [{0: (0, 0, 3), 1: (1, 0, 2)}, {1: (1, 2, 2)}]
    assert steps == [([0, 1], [3, -1]), ([-1, 1], [-1, 104])]


def test_schedule_chunk_of_one():
    steps, feeds = _drive([2, 1], [2, 1], 2, 1, _tok)
    assert feeds == [{0: (0, 0, 1)}, {0: (0, 1, 1)}, {1: (1, 0, 1)}]
    assert steps == [([0, 1], [-1, -1]), ([0, 1], [2, -1]), ([0, 1], [3, 101])]


def test_schedule_budget_of_zero():
    steps, feeds = _drive([2, 3, 1], [0, 1, 1], 1, 4, _tok)
    # request 0 never takes a row; request 2 waits for the row request 1 frees
    assert feeds == [{0: (1, 0, 3)}, {0: (2, 0, 1)}]
    assert steps == [([1], [103]), ([2], [201])]


def test_schedule_stop_while_another_row_prefills():
    stop = 5

    def tokens(r, p):
        return stop if (r, p) == (0, 3) else _tok(r, p)
    steps, feeds = _drive([2, 6, 1], [9, 2, 1], 2, 2, tokens, stops=[stop])
    assert feeds == [{0: (0, 0, 2)}, {1: (1, 0, 2)}, {1: (1, 2, 2)}, {1: (1, 4, 2)}, {0: (2, 0, 1)}]
    assert steps[:3] == [([0, 1], [2, -1]), ([0, 1], [5, -1]), ([2, 1], [-1, -1])]
    # the stop frees row 0 for request 2; the chunk goes to request 1 first (lower id) until its prompt is done
    assert steps[3:] == [([2, 1], [-1, 106]), ([2, 1], [201, 107])]


def test_feed_order_is_request_order():
    n = chunked.feed([3, 1, -1, 2], [5, 5, 0, 5], [0, 4, 0, 5], 3)
    assert n.tolist() == [2, 1, 0, 0]                 # request 1 (row 1) first, request 3 (row 0) the rest; row 3 decodes


@pytest.mark.parametrize("C", [0, -1, 1.5, True, "2"])
def test_bad_chunk(C):
    m = _model("cpu")
    with pytest.raises(ValueError):
        m.serve(_prompts([2, 3]), 2, prefill_chunk=C)


def test_chunk_past_the_row_limit():
    m = _model("cpu")
    with pytest.raises(ValueError):
        m.serve(_prompts([2, 3]), 2, slots=2, prefill_chunk=255)
    m.serve(_prompts([2, 3]), 2, slots=2, prefill_chunk=254)    # (checked when called, nothing runs yet)


@pytest.mark.parametrize("C", [1, 3, 17, 256 - 3])
@pytest.mark.parametrize("kw", [{}] + SAMPLED[:2])
def test_cpu_matches_serve(C, kw):
    prompts = _prompts(LENS, seed=1)
    want = _serve_all(_model("cpu"), prompts, BUDGETS, slots=3, **kw)
    got = _serve_all(_model("cpu"), prompts, BUDGETS, slots=3, prefill_chunk=C, **kw)
    if C >= sum(LENS):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    else:
        # a prompt pass's padding may round differently from serve's: the margin rule against generate_ragged
        ref, logits = _reference(prompts, BUDGETS, **kw)
        _check(got, _want(ref, BUDGETS), logits, prompts, kw, exact=False)


@pytest.mark.parametrize("kw", [{}, SAMPLED[0]])
def test_large_chunk_yields_serve_steps(kw):
    prompts = _prompts(LENS, seed=4)
    want = _stream(_model("cpu"), prompts, BUDGETS, slots=2, stop_ids=[7], **kw)
    got = _stream(_model("cpu"), prompts, BUDGETS, slots=2, stop_ids=[7], prefill_chunk=256 - 2, **kw)
    assert len(got) == len(want)
    for (gr, gt), (wr, wt) in zip(got, want):
        assert np.array_equal(gr, wr) and np.array_equal(gt, wt)


def test_small_chunk_delays_first_tokens():
    prompts = _prompts([6, 6], seed=5)
    steps = _stream(_model("cpu"), prompts, [2, 2], slots=2, prefill_chunk=4)
    assert [t.tolist() for _, t in steps][:2] == [[-1, -1], [steps[1][1][0], -1]]
    assert steps[1][1][0] >= 0 and steps[2][1][1] >= 0


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("slots,C", [(2, 1), (3, 4), (5, 64), (12, 16)])
@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
def test_emulated_matches_cpu(emulated_hip, graphs, slots, C, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    lens = [1 + (5 * i) % 9 for i in range(13)]
    budgets = [(3 * i) % 8 for i in range(13)]
    prompts = _prompts(lens, seed=3)
    ref, logits = _reference(prompts, budgets, **kw)
    m = _model("hip:0", B=12)
    counters()
    got = _serve_all(m, prompts, budgets, slots=slots, prefill_chunk=C, stop_ids=[9], **kw)
    c = counters()
    _check(got, _want(ref, budgets, stops=[9]), logits, prompts, kw, exact=False)
    assert c[33] > 0 and c[31] > 0                                # the extend launches and the wide product ran
    st = m._decode_st
    assert st["serve"] and st["B"] == slots and st["mixed"]["C"] == C


def test_emulated_without_chunk_is_unchanged(emulated_hip):
    Graph.clear()
    prompts = _prompts(LENS, seed=2)
    m = _model("hip:0")
    counters()
    _serve_all(m, prompts, BUDGETS, slots=3)
    c = counters()
    assert c[33] == 0 and c[30] > 0
    assert "mixed" not in m._decode_st
    assert all(len(k) == 2 for k in m._decode_st["graphs"])


def test_emulated_refusing_library_follows_the_schedule(emulated_hip, monkeypatch):
    """Without the mixed entries the prompt passes run when the schedule completes prompts; tokens as on `cpu`."""
    Graph.clear()
    monkeypatch.setattr(Llama, "wide_decode", False)
    prompts = _prompts(LENS, seed=2)
    ref, logits = _reference(prompts, BUDGETS)
    m = _model("hip:0")
    counters()
    got = _serve_all(m, prompts, BUDGETS, slots=3, prefill_chunk=2)
    c = counters()
    _check(got, _want(ref, BUDGETS), logits, prompts, {}, exact=False)
    assert c[33] == 0 and c[30] > 0
