"""Token log-probabilities on a real MI355X: pdn_logprobs_rows_f32 against the statement of llm/logprobs.py (ids exact,
values within 1 float32 ulp: the float64 exp / log of the device and of NumPy may differ in their last bits, and the
chunked log-sum-exp sums in another order), the tick form's records identical over two replays, launch counter 36, and
`generate`, `generate_ragged`, `serve` (plain and chunked) and `score` end to end against the `cpu` device on the narrow
(<= 8 rows) and the wide step.  Greedy runs follow the first-difference margin rule of tests/test_serve_gpu.py, read off
the `cpu` run's own top two logprobs; sampled runs must agree token for token.  Where the tokens agree the values are
within 1e-4 (the paths run different fp32 GEMMs) and every rank separated from its neighbours by more than that has the
same id.  On the device the tokens with logprobs on equal those with logprobs off, and launch counter 36 moves during
the decode steps themselves (after the prompt pass has been yielded)."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import logprobs as lp_np
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, logprobs_chunks as chunks

pytestmark = pytest.mark.gpu
f32 = np.float32
VOCAB = 1000                                     # (a multiple of 4: the graph-replayed step)
PEN = dict(repetition_penalty=1.6, presence_penalty=0.8, frequency_penalty=0.3)
SAMPLED = dict(temperature=0.9, top_p=0.92, seed=31)


def _case(B, V, seed):
    rng = np.random.default_rng(seed)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    z[:, ::97] = 0.0
    z[:, 5::131] = -0.0
    z[:, 7::101] = -np.inf
    z[:, 3::389] = z[:, :1]                                          # ties with column 0
    z[:, 13:16] = z.max(1, keepdims=True)                            # tied maxima
    tok = rng.integers(0, V, B).astype(np.int64)
    tok[1::3] = -1                                                   # rows that yielded nothing
    return z, tok


def _ulps(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    both = np.isnan(a) & np.isnan(b)
    same = (a == b) | both
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(same, 0, d).max(initial=0)


@pytest.mark.parametrize("V", [32000, 1001])
@pytest.mark.parametrize("B", [1, 8, 64, 256])
def test_rows_entry_matches_statement(hip, B, V):
    L = _lib.lib()
    assert L.query("pdn_logprobs_chunks", V) == chunks(V)
    z, tok = _case(B, V, B + V)
    full = lp_np.rows(z, tok, 20)
    Z, T = hip.from_numpy(z), hip.from_numpy(tok)
    for n in (0, 1, 5, 20):
        work = hip.zeros((L.query("pdn_logprobs_work_bytes", B, V, n) // 8 + 2,), np.int64)
        TOK = hip.from_numpy(np.full(B, 7.0, f32))
        IDS = hip.from_numpy(np.full((B, max(n, 1)), -7, np.int64))
        TOP = hip.from_numpy(np.full((B, max(n, 1)), 7.0, f32))
        L.call("pdn_logprobs_rows_f32", Z._ptr, V, B, V, n, T._ptr, TOK._ptr, IDS._ptr, TOP._ptr, work._ptr,
               hip.stream())
        assert _ulps(TOK.get(), full.token) <= 1
        assert np.isnan(TOK.get()[tok < 0]).all()
        if n:
            assert np.array_equal(IDS.get(), full.top_ids[:, :n])
            assert _ulps(TOP.get(), full.top_logprobs[:, :n]) <= 1


def _model(dev, B):
    np.random.seed(8)
    m = Llama(VOCAB, 96, 2, 128, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(VOCAB, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to(dev) if dev != "cpu" else m


def _prompts(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, VOCAB, n) for n in lens]


def _collect(it):
    """(ids, token, top_ids, top) stacked over the steps, and launch counter 36 over the steps after the first (the
    decode steps: the prompt pass's entry call is not counted)."""
    out, c36 = [], 0
    for i, (t, lp) in enumerate(it):
        out.append((t.numpy().reshape(-1).copy(), lp.token.reshape(-1).copy(), lp.top_ids.copy(),
                    lp.top_logprobs.copy()))
        if i == 0:
            counters()
    c36 = counters()[36]
    return [np.stack([o[k] for o in out], 1) for k in range(4)], c36


def _run(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn(m)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


GAP = 1e-4      # the margin rule's 1e-5 in logits, read off float32 logprobs of magnitude ~20 (a few ulps of 1.9e-6 each)


def _agree_row(ids_g, ids_w, lp_g, lp_w, ti_g, ti_w, tv_g, tv_w, greedy, what):
    """One row's steps: equal tokens up to the first difference, which a greedy run may show only where the `cpu`
    run's top two logprobs lie within GAP (needs n >= 2); values and separated ranks up to it."""
    n_ = min(len(ids_g), len(ids_w))
    diff = np.flatnonzero(ids_g[:n_] != ids_w[:n_])
    k = int(diff[0]) if diff.size else n_
    if k < n_:
        assert greedy, f"{what}: a sampled run differs at step {k}"
        gap = float(tv_w[k, 0]) - float(tv_w[k, 1])
        assert gap < GAP, f"{what}: step {k} differs at a margin of {gap}"
    np.testing.assert_allclose(lp_g[:k], lp_w[:k], atol=1e-4, err_msg=what)
    np.testing.assert_allclose(tv_g[:k], tv_w[:k], atol=1e-4, err_msg=what)
    tv = np.asarray(tv_w[:k], np.float64)
    n = tv.shape[1]
    sep = np.ones(tv.shape, bool)
    with np.errstate(invalid="ignore"):
        if n > 1:
            sep[:, 1:] &= (tv[:, :-1] - tv[:, 1:]) > GAP
            sep[:, :-1] &= (tv[:, :-1] - tv[:, 1:]) > GAP
    assert ((ti_g[:k] == ti_w[:k]) | ~sep).all(), what
    return k


def _agree(got, want, greedy):
    for b in range(got[0].shape[0]):
        _agree_row(got[0][b], want[0][b], got[1][b], want[1][b], got[2][b], want[2][b], got[3][b], want[3][b], greedy,
                   f"row {b}")


@pytest.mark.parametrize("B,kw", [(1, {}), (4, SAMPLED), (8, PEN), (24, {}), (64, SAMPLED)])
def test_generate_ragged_against_cpu(hip, B, kw):
    Graph.clear()
    prompts = _prompts([1 + (3 * i) % 9 for i in range(B)], seed=B)
    want, _ = _run(_model("cpu", B), lambda m: _collect(m.generate_ragged(prompts, 10, logprobs=5, **kw)))
    m = _model("hip:0", B)
    got, c36 = _run(m, lambda m: _collect(m.generate_ragged(prompts, 10, logprobs=5, **kw)))
    assert c36 > 0 and m._decode_st["lp_n"] == 5 and m._decode_st["ok"]      # (the replayed step's tick form)
    _agree(got, want, "temperature" not in kw)
    counters()
    plain = _run(m, lambda m: np.stack([t.numpy().reshape(-1) for t in m.generate_ragged(prompts, 10, **kw)], 1))
    assert np.array_equal(plain, got[0]) and counters()[36] == 0
    again, _ = _run(m, lambda m: _collect(m.generate_ragged(prompts, 10, logprobs=5, **kw)))
    assert all(np.array_equal(a.view(np.int32) if a.dtype == f32 else a, b.view(np.int32) if b.dtype == f32 else b)
               for a, b in zip(got, again))                        # two replayed runs: the same bits


@pytest.mark.parametrize("B", [2, 8, 16])
def test_generate_against_cpu(hip, B):
    Graph.clear()
    ids = np.stack(_prompts([6] * B, seed=40 + B))
    want, _ = _run(_model("cpu", B), lambda m: _collect(m.generate(ids, 6 + 9, logprobs=20)))
    got, c36 = _run(_model("hip:0", B), lambda m: _collect(m.generate(ids, 6 + 9, logprobs=20)))
    assert c36 > 0
    _agree(got, want, True)
    assert np.array_equal(got[2][:, :, 0], got[0]) and np.array_equal(got[3][:, :, 0], got[1])   # the pick is rank 0
    # n = 0 and n = 5 on the device: the same tokens, the same token values bit for bit
    for n in (0, 5):
        other, _ = _run(_model("hip:0", B), lambda m: _collect(m.generate(ids, 6 + 9, logprobs=n)))
        assert np.array_equal(other[0], got[0]) and np.array_equal(other[1].view(np.int32), got[1].view(np.int32))
        assert other[2].shape[2] == n and np.array_equal(other[2], got[2][:, :, :n])


def test_generic_step_counts(hip, monkeypatch):
    Graph.clear()
    ids = np.stack(_prompts([5] * 3, seed=50))
    m = _model("hip:0", 3)
    monkeypatch.setattr(Llama, "_decode_plan", lambda self, *a, **k: None)          # the generic launches
    got, c36 = _run(m, lambda m: _collect(m.generate(ids, 5 + 6, logprobs=3)))
    assert c36 == 5                                                 # one entry call per generic decode step
    want, _ = _run(_model("cpu", 3), lambda m: _collect(m.generate(ids, 5 + 6, logprobs=3)))
    _agree(got, want, True)


@pytest.mark.parametrize("S,chunk", [(3, None), (3, 4), (12, None), (12, 5)])
def test_serve_against_cpu(hip, S, chunk):
    Graph.clear()
    N = S + 5
    prompts = _prompts([1 + (5 * i) % 7 for i in range(N)], seed=60 + S)
    budgets = [2 + (3 * i) % 6 for i in range(N)]
    want = _run(_model("cpu", N), lambda m: m.serve_all(prompts, budgets, slots=S, prefill_chunk=chunk, logprobs=4))
    m = _model("hip:0", N)
    got, c36 = [], []

    def serve(m):
        steps = []
        for i, step in enumerate(m.serve(prompts, budgets, slots=S, prefill_chunk=chunk, logprobs=4)):
            steps.append(step)
            if i == 0:
                counters()
        c36.append(counters()[36])
        return steps
    steps = _run(m, serve)
    assert c36[0] > 0 and m._decode_st["lp_n"] == 4                 # entry calls during the decode steps
    got = [([], []) for _ in prompts]
    for reqs, toks, lp in steps:
        for b, (r, t) in enumerate(zip(reqs, toks)):
            if r >= 0 and t >= 0:
                got[r][0].append(int(t))
                got[r][1].append((lp.token[b], lp.top_ids[b], lp.top_logprobs[b]))
    plain = _run(_model("hip:0", N), lambda m: m.serve_all(prompts, budgets, slots=S, prefill_chunk=chunk))
    for r, ((tg, lg), (tw, lw), tp) in enumerate(zip(got, want, plain)):
        tg = np.array(tg, np.int64)
        assert np.array_equal(tg, tp)
        if not tg.size:
            continue
        lp_g = np.array([e[0] for e in lg], f32)
        ti_g = np.array([e[1] for e in lg], np.int64)
        tv_g = np.array([e[2] for e in lg], f32)
        _agree_row(tg, tw, lp_g, lw.token, ti_g, lw.top_ids, tv_g, lw.top_logprobs, True, f"request {r}")


def test_score_against_cpu_and_generation(hip):
    seq = np.random.default_rng(70).integers(0, VOCAB, (3, 20))
    want = _model("cpu", 1).score(seq, 5)
    m = _model("hip:0", 1)
    counters()
    got = m.score(seq, 5)
    assert counters()[36] > 0 and m._train
    np.testing.assert_allclose(got.token, want.token, atol=1e-4)
    np.testing.assert_allclose(got.top_logprobs, want.top_logprobs, atol=1e-4)
    # generation's first token comes from the prompt's causal pass: score of prompt + that token gives its value
    ids = seq[:, :8]
    first, _ = _run(_model("hip:0", 3), lambda m: _collect(m.generate(ids, 8 + 1, logprobs=5)))
    seq2 = np.concatenate([ids, first[0]], 1)
    s2 = m.score(seq2, 5)
    np.testing.assert_allclose(s2.token[:, -1], first[1][:, 0], atol=1e-4)
    np.testing.assert_allclose(s2.top_logprobs[:, -1], first[3][:, 0], atol=1e-4)
