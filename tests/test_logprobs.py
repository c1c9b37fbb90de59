"""Token log-probabilities (`logprobs=` of `generate`, `generate_ragged`, `serve`, `serve_all`; `Llama.score`) on the
CPU: the statement of llm/logprobs.py by hand cases, the `cpu` device against a hand loop of `forward_logits` plus the
statement, `score` against generation, argument errors, and the emulated C ABI with the entry points of
tests/abi_emulator/_logprobs.py (the graph-replayed steps, with and without graphs) against `cpu`."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core import Tensor
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import beam, logprobs as lp_np, penalties
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters
from tests.test_ragged import SAMPLED, V, _gen, _model, _prompts, _ragged

PEN = dict(repetition_penalty=1.8, presence_penalty=0.7, frequency_penalty=0.4)


# -- the statement ----------------------------------------------------------------------------------------------------
def test_order_ties_and_neg_inf():
    z = np.array([[1.0, 3.0, -np.inf, 3.0, 0.0, -np.inf]], np.float32)
    lp = lp_np.rows(z, [3], 6)
    assert lp.top_ids.tolist() == [[1, 3, 0, 4, 2, 5]]           # ties to the lower id, -inf last (lower id first)
    want = beam.log_softmax_rows(z)[0]
    assert np.array_equal(lp.top_logprobs[0], want[[1, 3, 0, 4, 2, 5]])
    assert lp.token[0] == want[3] and lp.top_logprobs[0, -1] == -np.inf


def test_ties_after_rounding_go_to_the_lower_id():
    # two different logits whose logps round to the same float32: ranked by logp, then id
    z = np.array([[0.001, 0.0010001, 40.0]], np.float32)
    lp = lp_np.rows(z, [0], 3)
    full = beam.log_softmax_rows(z)[0]
    assert z[0, 1] > z[0, 0] and full[0] == full[1] and lp.top_ids.tolist() == [[2, 0, 1]]


def test_n_zero_and_skipped_rows():
    z = np.random.default_rng(0).standard_normal((3, 10)).astype(np.float32)
    lp = lp_np.rows(z, [2, -1, 9], 0)
    assert lp.top_ids.shape == (3, 0) and lp.top_logprobs.shape == (3, 0)
    assert np.isnan(lp.token[1]) and lp.token[0] == beam.log_softmax_rows(z)[0, 2]
    lp = lp_np.rows(z, [2, -1, 9], 4)
    assert lp.top_ids[1].tolist() == [-1] * 4 and np.isnan(lp.top_logprobs[1]).all()


def test_more_than_v_leaves_the_rest_unset():
    lp = lp_np.rows(np.zeros((1, 3), np.float32), [0], 5)
    assert lp.top_ids.tolist() == [[0, 1, 2, -1, -1]] and np.isnan(lp.top_logprobs[0, 3:]).all()


def test_records_round_trip():
    z = np.random.default_rng(1).standard_normal((4, 30)).astype(np.float32)
    z[0, 3] = -np.inf
    lp = lp_np.rows(z, [3, -1, 0, 29], 5)
    back = lp_np.from_records(lp_np.to_records(lp), 5)
    for a, b in zip(lp, back):
        assert np.array_equal(np.asarray(a).view(np.int32 if a.dtype == np.float32 else np.int64),
                              np.asarray(b).view(np.int32 if b.dtype == np.float32 else np.int64))
    assert (lp_np.to_records(lp) != lp_np.UNSET).all()


@pytest.mark.parametrize("bad", [-1, 21, True, 1.0, "3", None])
def test_check_n(bad):
    with pytest.raises(ValueError):
        lp_np.check_n(bad, allow_none=False)
    assert lp_np.check_n(None) is None and lp_np.check_n(0) == 0 and lp_np.check_n(np.int64(20)) == 20


# -- the `cpu` device ---------------------------------------------------------------------------------------------------
def _collect(it):
    """(ids (B, steps), token (B, steps), top_ids (B, steps, n), top (B, steps, n)) of a generate-style iterator."""
    ids, tok, ti, tv = [], [], [], []
    try:
        with pdn.no_grad():
            for t, lp in it:
                ids.append(t.numpy().reshape(-1).copy())
                tok.append(lp.token.reshape(-1))
                ti.append(lp.top_ids)
                tv.append(lp.top_logprobs)
    finally:
        pdn.autograd.set_grad_enabled(True)
    return np.stack(ids, 1), np.stack(tok, 1), np.stack(ti, 1), np.stack(tv, 1)


def _gen_lp(m, ids, total, n, **kw):
    m.eval()
    try:
        return _collect(m.generate(np.asarray(ids), total, logprobs=n, **kw))
    finally:
        m.train(True)


def _ragged_lp(m, prompts, steps, n, **kw):
    m.eval()
    try:
        return _collect(m.generate_ragged(prompts, steps, logprobs=n, **kw))
    finally:
        m.train(True)


def _hand(prompts, got, n, pen=None):
    """Row by row on a fresh model, feeding the tokens generation yielded: forward_logits, the penalties, the
    statement -> (token (B, steps), top_ids, top) with nan / -1 where a row yielded nothing."""
    B, steps = got.shape
    tok = np.full((B, steps), np.nan, np.float32)
    ti = np.full((B, steps, n), -1, np.int64)
    tv = np.full((B, steps, n), np.nan, np.float32)
    try:
        with pdn.no_grad():
            for b, q in enumerate(prompts):
                m = _model("cpu", B=1)
                m.eval()
                seq, gen = [int(t) for t in q], []
                for i in range(steps):
                    t = int(got[b, i])
                    if t < 0:
                        break
                    feed, at = (seq, 0) if i == 0 else (seq[-1:], len(q) + i)
                    z = np.asarray(m.forward_logits(Tensor(np.array([feed], np.int64), dtype=np.int64), at).numpy(),
                                   np.float32)[0, -1][None]
                    if pen is not None:
                        c = np.bincount(np.array(gen, np.int64), minlength=V)
                        z = penalties.penalize(z, c[None], penalties.seen_rows([q], V), *pen)
                    lp = lp_np.rows(z, [t], n)
                    tok[b, i], ti[b, i], tv[b, i] = lp.token[0], lp.top_ids[0], lp.top_logprobs[0]
                    gen.append(t)
                    seq.append(t)
    finally:
        pdn.autograd.set_grad_enabled(True)
    return tok, ti, tv


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _agree(got, want):
    """(ids, token, top_ids, top) of two runs: ids and ranks exact, values within 1e-4 (other fp32 GEMMs)."""
    return (_same(got[0], want[0]) and _close(got[1], want[1]) and _same(got[2], want[2])
            and _close(got[3], want[3]))


def _close(a, b, atol=1e-4):
    """Values of the batched `cpu` pass against the one-row hand loop: the same fp32 GEMMs on other shapes."""
    return np.allclose(np.asarray(a), np.asarray(b), rtol=0, atol=atol, equal_nan=True)


@pytest.mark.parametrize("kw", [{}, SAMPLED[1], PEN])
def test_cpu_generate_ragged_values_equal_hand_loop(kw):
    prompts = _prompts([3, 1, 6, 2], seed=4)
    ids, tok, ti, tv = _ragged_lp(_model("cpu"), prompts, 8, 5, stop_ids=[7], **kw)
    assert np.array_equal(ids, _ragged(_model("cpu"), prompts, 8, stop_ids=[7], **kw))
    pen = penalties.check_args(**PEN) if kw is PEN else None
    want = _hand(prompts, ids, 5, pen)
    assert _close(tok, want[0]) and _same(ti, want[1]) and _close(tv, want[2])


@pytest.mark.parametrize("kw", [{}, SAMPLED[0], PEN])
def test_cpu_generate_values_equal_hand_loop(kw):
    ids0 = np.stack(_prompts([4, 4, 4], seed=5))
    ids, tok, ti, tv = _gen_lp(_model("cpu"), ids0, 4 + 7, 3, **kw)
    assert np.array_equal(ids, _gen(_model("cpu"), ids0, 4 + 7, **kw))
    pen = penalties.check_args(**PEN) if kw is PEN else None
    want = _hand(list(ids0), ids, 3, pen)
    assert _close(tok, want[0]) and _same(ti, want[1]) and _close(tv, want[2])
    if not kw:                                                      # greedy: the first ranked token is the pick
        assert np.array_equal(ti[:, :, 0], ids) and np.array_equal(tv[:, :, 0], tok)


def test_cpu_n_zero_yields_only_the_token():
    ids0 = np.stack(_prompts([3, 3], seed=6))
    ids, tok, ti, tv = _gen_lp(_model("cpu"), ids0, 3 + 5, 0)
    assert ti.shape == (2, 5, 0) and tv.shape == (2, 5, 0) and np.isfinite(tok).all()


def _serve_lp(m, prompts, budgets, n, **kw):
    m.eval()
    try:
        with pdn.no_grad():
            return m.serve_all(prompts, budgets, logprobs=n, **kw)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


@pytest.mark.parametrize("chunk", [None, 3])
@pytest.mark.parametrize("kw", [{}, SAMPLED[2], PEN])
def test_cpu_serve_all_equals_generate_ragged(kw, chunk):
    prompts = _prompts([3, 1, 6, 2, 4], seed=8)
    budgets = [6, 3, 5, 1, 4]
    got = _serve_lp(_model("cpu", B=5), prompts, budgets, 4, slots=2, prefill_chunk=chunk, stop_ids=[9], **kw)
    ids, tok, ti, tv = _ragged_lp(_model("cpu", B=5), prompts, max(budgets), 4, stop_ids=[9], **kw)
    m = _model("cpu", B=5)
    m.eval()
    plain = m.serve_all(prompts, budgets, slots=2, prefill_chunk=chunk, stop_ids=[9], **kw)
    for r, (t, lp) in enumerate(got):
        k = len(t)
        assert t.tolist() == plain[r].tolist() and t.tolist() == ids[r, :k].tolist()
        assert lp.token.shape == (k,) and lp.top_ids.shape == (k, 4) and lp.top_logprobs.shape == (k, 4)
        assert _close(lp.token, tok[r, :k]) and _same(lp.top_ids, ti[r, :k]) and _close(lp.top_logprobs, tv[r, :k])


def test_cpu_serve_steps_mark_empty_slots():
    prompts = _prompts([2, 3, 4], seed=9)
    m = _model("cpu", B=3)
    m.eval()
    for chunk in (None, 2):
        for reqs, toks, lp in m.serve(prompts, [3, 2, 4], slots=2, logprobs=2, prefill_chunk=chunk):
            assert lp.token.shape == (2,) and lp.top_ids.shape == (2, 2)
            none = toks < 0
            assert np.isnan(lp.token[none]).all() and (lp.top_ids[none] == -1).all()
            assert np.isfinite(lp.token[~none]).all()


def test_cpu_score_equals_generation():
    prompts = _prompts([4, 4], seed=10)
    ids, tok, ti, tv = _gen_lp(_model("cpu"), np.stack(prompts), 4 + 6, 5)
    m = _model("cpu")
    m.eval()
    seq = np.concatenate([np.stack(prompts), ids], 1)
    got = m.score(seq, logprobs=5)
    assert got.token.shape == (2, 9) and got.top_ids.shape == (2, 9, 5)
    assert not m._train                                            # the mode is restored
    # the prompt pass's token: the same causal pass.  (Later steps of `generate` feed the token of position p - 1 at
    # position p, as the reference does, so they are not the values of a pass over prompt + generated.)
    np.testing.assert_allclose(got.token[:, 3], tok[:, 0], atol=1e-4)
    np.testing.assert_allclose(got.top_logprobs[:, 3], tv[:, 0], atol=1e-4)
    assert np.array_equal(got.top_ids[:, 3], ti[:, 0])
    m.train(True)
    again = m.score(seq)
    assert m._train and again.top_ids.shape == (2, 9, 0)
    np.testing.assert_allclose(again.token, got.token, atol=1e-5)


def test_cpu_score_ignores_max_batch_size_and_cache():
    m = _model("cpu", B=1)
    seq = np.random.default_rng(11).integers(0, V, (3, 12))
    cache = m.layers[0].attention.cache_k.numpy().copy()
    got = m.score(seq, 2)
    assert got.token.shape == (3, 11) and np.array_equal(m.layers[0].attention.cache_k.numpy(), cache)
    for b in range(3):
        z = np.asarray(m.forward_logits(Tensor(seq[b:b + 1, :-1], dtype=np.int64), 0).numpy(), np.float32)[0]
        want = lp_np.rows(z, seq[b, 1:], 2)
        np.testing.assert_allclose(got.token[b], want.token, atol=1e-5)


# -- arguments --------------------------------------------------------------------------------------------------------
BAD = [-1, 21, True, 2.0, "1"]


@pytest.mark.parametrize("bad", BAD)
def test_bad_n_raises_before_any_launch(emulated_hip, bad):
    from pydynet_amd import _lib
    m = _model("hip:0")
    prompts = _prompts([2, 3])
    n0 = len(_lib._LIB.calls)
    for call in (lambda: m.generate(np.stack(_prompts([3, 3])), 8, logprobs=bad),
                 lambda: m.generate_ragged(prompts, 4, logprobs=bad),
                 lambda: m.serve(prompts, 4, logprobs=bad),
                 lambda: m.serve(prompts, 4, prefill_chunk=2, logprobs=bad),
                 lambda: m.serve_all(prompts, 4, logprobs=bad),
                 lambda: m.score(np.stack(_prompts([3, 3])), bad)):
        with pytest.raises(ValueError):
            call()
    assert len(_lib._LIB.calls) == n0


def test_score_arguments(emulated_hip):
    from pydynet_amd import _lib
    m = _model("hip:0")
    n0 = len(_lib._LIB.calls)
    for bad in (np.zeros((2, 1), np.int64), np.zeros(5, np.int64), np.full((1, 3), V), np.full((1, 3), -1)):
        with pytest.raises(ValueError):
            m.score(bad)
    with pytest.raises(ValueError):
        m.score(np.zeros((1, 3), np.int64), None)
    assert len(_lib._LIB.calls) == n0


def test_logprobs_refused_with_speculation():
    m = _model("cpu")
    with pytest.raises(ValueError, match="speculate"):
        m.generate_ragged(_prompts([2, 3]), 4, speculate=2, logprobs=0)


# -- the emulated HIP path --------------------------------------------------------------------------------------------
RUNTIME = ("pdn_malloc", "pdn_free", "pdn_set_device", "pdn_compute_stream", "pdn_fill", "pdn_kernel_counters",
           "pdn_memcpy")


def test_default_launches_unchanged(emulated_hip):
    from pydynet_amd import _lib
    Graph.clear()
    ids = np.stack(_prompts([4, 4], seed=10))
    _lib._LIB.calls.clear()
    counters()
    base = _gen(_model("hip:0"), ids, 14)
    c0, calls0 = counters(), list(_lib._LIB.calls)
    _lib._LIB.calls.clear()
    again = _gen(_model("hip:0"), ids, 14, logprobs=None)
    c1, calls1 = counters(), list(_lib._LIB.calls)
    calls0, calls1 = ([c for c in cl if not c.startswith(RUNTIME)] for cl in (calls0, calls1))
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[36] == 0
    assert not any("logprobs" in c for c in calls0)
    m = _model("hip:0")
    _ragged(m, _prompts([3, 5, 2], seed=11), 6)
    assert m._decode_st["lp_n"] is None and "lp_box" not in m._decode_st
    assert len(m._decode_st["key"]) == 11                          # (the key of a plan without logprobs)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw", [(3, {}), (5, SAMPLED[1]), (12, {}), (10, PEN)])
def test_emulated_generate_ragged_equals_cpu(emulated_hip, graphs, B, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    prompts = _prompts([1 + (3 * i) % 7 for i in range(B)], seed=12)
    want = _ragged_lp(_model("cpu", B=max(B, 5)), prompts, 9, 5, stop_ids=[5], **kw)
    m = _model("hip:0", B=max(B, 5))
    counters()
    got = _ragged_lp(m, prompts, 9, 5, stop_ids=[5], **kw)
    c = counters()
    assert _agree(got, want)
    assert c[36] > 0 and m._decode_st["lp_n"] == 5
    plain = _ragged(_model("hip:0", B=max(B, 5)), prompts, 9, stop_ids=[5], **kw)
    assert np.array_equal(plain, got[0])


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("B,kw,n", [(3, {}, 0), (2, SAMPLED[2], 20), (12, {}, 3)])
def test_emulated_generate_equals_cpu(emulated_hip, graphs, B, kw, n, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    ids = np.stack(_prompts([5] * B, seed=13))
    want = _gen_lp(_model("cpu", B=max(B, 5)), ids, 5 + 10, n, **kw)
    counters()
    got = _gen_lp(_model("hip:0", B=max(B, 5)), ids, 5 + 10, n, **kw)
    assert _agree(got, want) and counters()[36] > 0


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("S,chunk,kw", [(3, None, {}), (3, 4, {}), (2, None, SAMPLED[1]), (10, None, PEN),
                                         (10, 3, SAMPLED[0])])
def test_emulated_serve_equals_cpu(emulated_hip, graphs, S, chunk, kw, monkeypatch):
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    N = S + 4
    prompts = _prompts([1 + (5 * i) % 6 for i in range(N)], seed=14)
    budgets = [2 + (3 * i) % 7 for i in range(N)]
    want = _serve_lp(_model("cpu", B=N), prompts, budgets, 4, slots=S, stop_ids=[7], prefill_chunk=chunk, **kw)
    counters()
    got = _serve_lp(_model("hip:0", B=N), prompts, budgets, 4, slots=S, stop_ids=[7], prefill_chunk=chunk, **kw)
    assert counters()[36] > 0
    for (t0, l0), (t1, l1) in zip(want, got):
        assert np.array_equal(t0, t1) and _agree((t0,) + tuple(l0), (t1,) + tuple(l1))


def test_emulated_score_equals_cpu(emulated_hip):
    seq = np.random.default_rng(15).integers(0, V, (3, 10))
    want = _model("cpu").score(seq, 6)
    m = _model("hip:0")
    counters()
    got = m.score(seq, 6)
    assert counters()[36] > 0
    np.testing.assert_allclose(got.token, want.token, atol=1e-5)
    np.testing.assert_allclose(got.top_logprobs, want.top_logprobs, atol=1e-5)


def test_emulated_speculate_with_logprobs_raises_before_any_launch(emulated_hip):
    from pydynet_amd import _lib
    m = _model("hip:0")
    n0 = len(_lib._LIB.calls)
    with pytest.raises(ValueError, match="speculate"):
        m.generate_ragged(_prompts([2, 3]), 4, speculate=3, logprobs=2)
    assert len(_lib._LIB.calls) == n0


@pytest.mark.parametrize("chunk", [None, 2])
def test_cpu_serve_all_n_zero(chunk):
    """n = 0 (token values only), with a request of budget 0 (no tokens: arrays of length 0)."""
    prompts = _prompts([2, 3, 4, 1], seed=16)
    budgets = [3, 0, 4, 2]
    got = _serve_lp(_model("cpu", B=4), prompts, budgets, 0, slots=2, prefill_chunk=chunk)
    with_n = _serve_lp(_model("cpu", B=4), prompts, budgets, 3, slots=2, prefill_chunk=chunk)
    for (t, lp), (t3, lp3), k in zip(got, with_n, budgets):
        assert t.size == k and np.array_equal(t, t3)
        assert lp.token.shape == (k,) and lp.top_ids.shape == (k, 0) and lp.top_logprobs.shape == (k, 0)
        assert np.array_equal(lp.token, lp3.token) and np.isfinite(lp.token).all()
    assert got[1][0].size == 0
