"""Prompt-lookup speculative decoding (`Llama.generate_ragged(..., speculate=k)`) on the CPU: the draft and accept rules of
llm/speculative.py by hand cases, the `cpu` device against `speculate=0`, argument errors, and the emulated C ABI with
the entry points of tests/abi_emulator/_extend.py (the graph-replayed pass, with and without graphs) against the
statement."""
import numpy as np
import pytest

from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import speculative
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, draft_np, remove
from tests.test_ragged import SAMPLED, V, _model, _prompts, _ragged


def _draft(h, k=4, left=100):
    return speculative.draft(np.array(h), k, left).tolist()


# -- the draft rule ---------------------------------------------------------------------------------------------------
def test_draft_no_match():
    assert _draft([1, 2, 3, 4, 5]) == []
    assert _draft([7]) == []


def test_draft_match_ending_one_before_the_suffix():
    # key (2, 3) at the end; h[1:3] == key and 1 + 2 < T: the draft is h[3:4] -- the one token before the suffix
    assert _draft([1, 2, 3, 2, 3]) == [2, 3]
    assert _draft([5, 9, 9]) == [9]               # n = 1: j = 1 (j + n < T), draft h[2:3]


def test_draft_longest_n_preferred_over_a_later_shorter_match():
    # the 3-gram (1, 2, 3) matches at j = 0, the 1-gram 3 later at j = 6: the 3-gram wins
    h = [1, 2, 3, 7, 8, 9, 3, 5, 1, 2, 3]
    assert _draft(h) == [7, 8, 9, 3]
    # among matches of one n the most recent
    assert _draft([4, 1, 4, 2, 4]) == [2, 4]


def test_draft_clipped_at_T_k_and_left():
    h = [1, 2, 3, 4, 1, 2, 3]
    assert _draft(h, k=16) == [4, 1, 2, 3]        # clipped at T
    assert _draft(h, k=2) == [4, 1]               # at k
    assert _draft(h, k=16, left=3) == [4, 1]      # at left - 1
    assert _draft(h, k=16, left=1) == []


# -- the accept rule --------------------------------------------------------------------------------------------------
def _accept(fed, picks, left=100, stops=()):
    y, a, hit = speculative.accept(fed, picks, left, stops)
    return y.tolist(), a, hit


def test_accept_all():
    assert _accept([5, 6, 7, 8], [6, 7, 8, 9]) == ([6, 7, 8, 9], 3, False)


def test_accept_none():
    assert _accept([5, 6, 7, 8], [1, 7, 8, 9]) == ([1], 0, False)
    assert _accept([5], [4]) == ([4], 0, False)


def test_accept_stop_inside_the_accepted_prefix():
    assert _accept([5, 6, 7, 8], [6, 7, 8, 9], stops=[7]) == ([6, 7], 3, True)


def test_accept_stop_as_the_bonus_token():
    assert _accept([5, 6, 7], [6, 7, 3], stops=[3]) == ([6, 7, 3], 2, True)
    assert _accept([5, 6, 7], [6, 2, 3], stops=[2]) == ([6, 2], 1, True)


def test_accept_budget():
    assert _accept([5, 6, 7], [6, 7, 3], left=2) == ([6, 7], 2, False)


# -- the `cpu` device: the streams of speculate=0 ---------------------------------------------------------------------
def _repetitive(lens, seed=0, period=4):
    rng = np.random.default_rng(seed)
    return [np.resize(rng.integers(0, V, period), n) for n in lens]


def _spec(m, prompts, n, k, **kw):
    got = _ragged(m, prompts, n, speculate=k, **kw)
    return got, dict(m.last_speculation)


@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_cpu_equals_plain(kw, k):
    prompts = _prompts([3, 1, 7, 2, 5], seed=1)
    want = _ragged(_model("cpu"), prompts, 12, **kw)
    got, c = _spec(_model("cpu"), prompts, 12, k, **kw)
    assert np.array_equal(got, want)
    assert c["tokens"] == int((want[:, 1:] >= 0).sum()) and c["accepted"] <= c["drafted"]


@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
def test_cpu_stop_ids(kw):
    prompts = _prompts([4, 2, 6, 3], seed=2)
    want = _ragged(_model("cpu"), prompts, 14, **kw)
    stops = sorted({int(want[0, 3]), int(want[2, 6])})
    want = _ragged(_model("cpu"), prompts, 14, stop_ids=stops, **kw)
    got, _ = _spec(_model("cpu"), prompts, 14, 4, stop_ids=stops, **kw)
    assert np.array_equal(got, want)
    assert (want == -1).any()


def test_cpu_budgets_of_one_and_two():
    prompts = _prompts([3, 5], seed=3)
    m = _model("cpu")
    assert list(m.generate_ragged(prompts, 0, speculate=4)) == [] and m.last_speculation == speculative.counts()
    for n in (1, 2):
        want = _ragged(_model("cpu"), prompts, n)
        got, c = _spec(_model("cpu"), prompts, n, 4)
        assert np.array_equal(got, want)
    assert c["passes"] == 1


def test_cpu_row_ending_at_the_last_cache_position():
    # seq 32: a prompt of 20 with 12 new tokens decodes its last step at position 31
    prompts = _repetitive([20, 4], seed=4)
    want = _ragged(_model("cpu"), prompts, 12)
    got, _ = _spec(_model("cpu"), prompts, 12, 6)
    assert np.array_equal(got, want)


def test_cpu_repetitive_history_takes_fewer_passes():
    # (seed 3: the greedy continuation falls into a loop the drafts predict)
    prompts = _repetitive([8], seed=3)
    want = _ragged(_model("cpu", B=1), prompts, 20)
    got, c = _spec(_model("cpu", B=1), prompts, 20, 4)
    assert np.array_equal(got, want)
    assert c["tokens"] == 19 and c["accepted"] > 0 and c["passes"] < c["tokens"]
    assert c["passes"] + c["accepted"] == c["tokens"]


# -- arguments --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [True, -1, 17, 2.0, "2", None])
def test_bad_speculate(bad):
    m = _model("cpu")
    with pytest.raises(ValueError):
        m.generate_ragged(_prompts([2, 3]), 4, speculate=bad)


def test_query_row_limit():
    m = _model("cpu", B=32)
    with pytest.raises(ValueError, match="256 query rows"):
        m.generate_ragged(_prompts([2] * 32), 4, speculate=8)
    m.generate_ragged(_prompts([2] * 32), 4, speculate=7)             # (checked when called, nothing runs yet)


def test_speculate_zero_runs_the_plain_decode():
    m = _model("cpu")
    _ragged(m, _prompts([2, 3]), 4)
    assert m.last_speculation is None


# -- the emulated HIP path --------------------------------------------------------------------------------------------
def test_draft_entry_edge_cases(emulated_hip):
    hist = np.zeros((4, 10), np.int32)
    hist[0, :5] = [1, 2, 3, 1, 2]
    hist[1, :3] = [5, 6, 7]
    hist[2, :6] = [4, 4, 4, 4, 4, 4]
    hist[3, :2] = [9, 9]
    tok, qpos, runs = draft_np(hist, [5, 3, 6, 2], [6, 4, -1, 3], [10, 10, 10, 1], 3)
    assert tok.reshape(4, 4).tolist() == [[2, 3, 1, 2], [7, 0, 0, 0], [0, 0, 0, 0], [9, 0, 0, 0]]
    assert qpos.reshape(4, 4).tolist() == [[6, 7, 8, 9], [4, -1, -1, -1], [-1] * 4, [3, -1, -1, -1]]
    assert runs.tolist() == [[0, 4, 6, 0], [4, 1, 4, 0], [8, 0, 0, 0], [12, 1, 3, 0]]


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,k,kw", [(1, 4, {}), (5, 2, {}), (3, 3, SAMPLED[1]), (12, 1, {})])
def test_emulated_matches_statement(emulated_hip, graphs, B, k, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    monkeypatch.setattr(Llama, "decode_ahead", False)
    Graph.clear()
    prompts = _repetitive([1 + (5 * i) % 9 for i in range(B)], seed=6)
    stops = [9]
    want, wc = _spec(_model("cpu", B=max(B, 5)), prompts, 10, k, stop_ids=stops, **kw)
    m = _model("hip:0", B=max(B, 5))
    counters()
    got, gc = _spec(m, prompts, 10, k, stop_ids=stops, **kw)
    c = counters()
    assert np.array_equal(got, want)
    assert gc == wc
    assert c[34] == 2 * gc["passes"] and c[33] > 0 and c[31] > 0    # one draft launch and one tick per pass
    assert m._spec_st["B"] == B and m._spec_st["k"] == k


def test_emulated_plan_is_reused(emulated_hip):
    Graph.clear()
    prompts = _repetitive([3, 5], seed=7)
    m = _model("hip:0")
    a, _ = _spec(m, prompts, 8, 3)
    st = m._spec_st
    b, _ = _spec(m, prompts, 8, 3)
    assert m._spec_st is st and np.array_equal(a, b)


def test_emulated_refusing_library_follows_the_statement(emulated_hip, monkeypatch):
    """Without the speculative entries the passes run on the generic rows step; tokens and counts as on `cpu`."""
    Graph.clear()
    from pydynet_amd import _lib
    remove(monkeypatch, _lib._LIB, "pdn_spec_draft_rows")
    prompts = _repetitive([3, 6, 2], seed=8)
    want, wc = _spec(_model("cpu"), prompts, 9, 3, stop_ids=[9])
    m = _model("hip:0")
    counters()
    got, gc = _spec(m, prompts, 9, 3, stop_ids=[9])
    c = counters()
    assert np.array_equal(got, want) and gc == wc
    assert c[34] == 0 and c[29] > 0
