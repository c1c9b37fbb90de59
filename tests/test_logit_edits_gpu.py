"""allowed_token_ids, logit_bias and min_new_tokens on a real MI355X: the entries of csrc/logit_edit.hip bit for bit against
the float32 statement (tests/abi_emulator/_logitedit.py over llm/logit_edits.py), the plan after a graph-replayed run, and
`generate`, `generate_ragged` and `serve` (plain and chunked) end to end against the `cpu` device under the
first-difference margin rule of tests/test_penalties_gpu.py, on the narrow (<= 8 rows) and the wide step."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import logit_edits as E
from pydynet_amd.llm import penalties
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import margin
from tests.abi_emulator._logitedit import edit_chunks as chunks, edit_np, edit_reset_np

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
PEN = dict(repetition_penalty=1.6, presence_penalty=0.8, frequency_penalty=0.3)
SAMPLED = dict(temperature=0.9, top_p=0.92, seed=31)
M = E.MAX_BIAS


def _counters():
    buf = (ctypes.c_int64 * 49)()
    _lib.lib().call("pdn_kernel_counters", buf, 49, 1)
    return [int(v) for v in buf]


def _state_case(B, V, seed):
    """Logit rows with zeros and infinities, and a packed state whose rows cycle through: allowed sets -- none, one token,
    everything but one token, a random half; bias tables -- none, one entry, MAX_BIAS entries (every token where V is
    smaller), entries on the first and last token of each chunk and of the row -- with bans (-inf) among the values."""
    rng = np.random.default_rng(seed)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    z[:, ::97] = 0.0
    z[:, 5::131] = -0.0
    z[:, 7::101] = -INF
    z[:, 11::211] = INF
    allow, bias = [], []
    edge = np.unique(np.array([0, 1023, 1024, 2047, 2048, V - 1025, V - 1024, V - 2, V - 1]) % V)
    for b in range(B):
        k = (b + seed) % 4
        allow.append(None if k == 0 else np.array([(b * 37 + V - 1) % V]) if k == 1
                     else np.delete(np.arange(V), (b * 53) % V) if k == 2 else np.flatnonzero(rng.random(V) < 0.5))
        k = (b // 4 + b + seed) % 4
        ids = (np.zeros(0, np.int64) if k == 0 else np.array([(b * 1023) % V]) if k == 1
               else rng.permutation(V)[:min(M, V)] if k == 2 else edge)
        vals = (3 * rng.standard_normal(ids.size)).astype(f32)
        vals[::5] = -INF
        vals[1::7] = 0.0
        bias.append((ids, vals))
    bits, on = E.allow_bits(allow, V)
    ids, vals, cnt = E.bias_tables(bias)
    pos = rng.integers(0, 60, B).astype(np.int32)
    pos[2::3] = -1                                                   # skipped rows stay untouched
    start = np.minimum(rng.integers(0, 60, B), np.maximum(pos, 0)).astype(np.int32)
    start[::2] = np.maximum(pos[::2], 0) - (np.arange(0, B, 2) % 5)   # generated 0 .. 4 around m = 3 (may go below 0: fine)
    stop = E.allow_bits([np.unique(np.concatenate([rng.integers(0, V, 6), [0, V - 1]]))], V)[0][0]
    return z, (bits, on, ids, vals, cnt), pos, start, stop


@pytest.mark.parametrize("V", [32000, 1001])
@pytest.mark.parametrize("B", [1, 8, 64, 256])
def test_edit_entries_bit_equal(hip, B, V):
    L = _lib.lib()
    z, state, pos, start, stop = _state_case(B, V, B + V)
    n = L.query("pdne_logit_edit_chunks", V)
    assert n == chunks(V)
    prm = hip.from_numpy(E.params_bytes(3))
    D = [hip.from_numpy(a) for a in state]
    ST, P, SP = hip.from_numpy(start), hip.from_numpy(pos), hip.from_numpy(stop)
    # the step's form: g = pos - start, the tick's stop bitmask, candidates
    want = z.copy()
    live, cv, ci = edit_np(want, 3, *state, pos - start, pos, stop)
    assert np.array_equal(live, pos >= 0) and not np.isnan(want).any()
    Z = hip.from_numpy(z)
    CV, CI = hip.from_numpy(np.full((B, n), 7.0, f32)), hip.from_numpy(np.full((B, n), -7, np.int32))
    L.call("pdne_logit_edit_step_f32", Z._ptr, V, B, V, prm._ptr, *(a._ptr for a in D), ST._ptr, P._ptr, 1, SP._ptr,
           CV._ptr, CI._ptr, hip.stream())
    got = Z.get()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[~live].view(np.int32), z[~live].view(np.int32))
    assert np.array_equal(CV.get()[live].view(np.int32), cv[live].view(np.int32))
    assert np.array_equal(CI.get()[live], ci[live])
    assert (CV.get()[~live] == 7.0).all() and (CI.get()[~live] == -7).all()
    for a, d in zip(state, D):                                       # the step only reads the state
        assert np.array_equal(d.get(), a)
    # the rows form: generated per row, no plan, no candidates
    gen = (np.arange(B) % 6).astype(np.int32)
    want = z.copy()
    edit_np(want, 3, *state, gen, pos, stop)
    Z, G = hip.from_numpy(z), hip.from_numpy(gen)
    L.call("pdne_logit_edit_rows_f32", Z._ptr, V, B, V, prm._ptr, *(a._ptr for a in D), G._ptr, P._ptr, SP._ptr, None,
           None, hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32))
    # ... every state pointer optional: the bias tables alone with candidates, then nothing at all
    want = z.copy()
    _, cv, ci = edit_np(want, 3, None, None, *state[2:])
    Z = hip.from_numpy(z)
    L.call("pdne_logit_edit_rows_f32", Z._ptr, V, B, V, prm._ptr, None, None, *(a._ptr for a in D[2:]), None, None, None,
           CV._ptr, CI._ptr, hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32))
    assert np.array_equal(CV.get().view(np.int32), cv.view(np.int32)) and np.array_equal(CI.get(), ci)
    Z = hip.from_numpy(z)
    L.call("pdne_logit_edit_rows_f32", Z._ptr, V, B, V, prm._ptr, None, None, None, None, None, None, None, SP._ptr, None,
           None, hip.stream())                                       # (generated NULL: 0 < m, the stop ids banned)
    want = z.copy()
    edit_np(want, 3, stop=stop)
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32)) and (want[:, 0] == -INF).all()


def test_step_entry_row_stride_and_shared_position(hip):
    """A logits row stride wider than V with the tail untouched, and the rectangular form (pos_per_row = 0: every row at
    pos[0]); a chunk of nothing but NaN yields (NaN, its first index), elsewhere a NaN never wins."""
    L = _lib.lib()
    B, V, rs = 5, 3001, 3072
    z, state, _, start, stop = _state_case(B, V, 5)
    z[3, 1024:2048] = np.nan
    z[4, 2050] = np.nan
    state[1][3:] = 0                                                 # (rows 3 and 4: no allowed set over the NaNs,
    state[4][3:] = 0                                                 #  no bias table, and past min_new_tokens)
    start[3:] = 0
    zz = np.full((B, rs), 3.0, f32)
    zz[:, :V] = z
    want = z.copy()
    _, cv, ci = edit_np(want, 2, *state, 30 - start, None, stop)
    assert np.isnan(cv[3, 1]) and ci[3, 1] == 1024 and not np.isnan(cv[4]).any()
    n = chunks(V)
    Z, ST, P, SP = hip.from_numpy(zz), hip.from_numpy(start), hip.from_numpy(np.array([30], np.int32)), hip.from_numpy(stop)
    D = [hip.from_numpy(a) for a in state]
    CV, CI = hip.from_numpy(np.zeros((B, n), f32)), hip.from_numpy(np.zeros((B, n), np.int32))
    prm = hip.from_numpy(E.params_bytes(2))
    L.call("pdne_logit_edit_step_f32", Z._ptr, rs, B, V, prm._ptr, *(a._ptr for a in D), ST._ptr, P._ptr, 0, SP._ptr,
           CV._ptr, CI._ptr, hip.stream())
    got = Z.get()
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got[:, :V]), ~ok) and np.array_equal(got[:, :V][ok].view(np.int32), want[ok].view(np.int32))
    assert (got[:, V:] == 3.0).all()
    assert np.array_equal(CI.get(), ci) and np.array_equal(np.isnan(CV.get()), np.isnan(cv))
    assert np.array_equal(CV.get()[~np.isnan(cv)].view(np.int32), cv[~np.isnan(cv)].view(np.int32))


@pytest.mark.parametrize("B,V", [(3, 32000), (70, 1001)])
def test_reset_entry(hip, B, V):
    L = _lib.lib()
    rng = np.random.default_rng(B)
    W = -(-V // 32)
    state = [rng.integers(-2 ** 31, 2 ** 31 - 1, (B, W)).astype(np.int32), rng.integers(0, 2, B).astype(np.int32),
             rng.integers(0, V, (B, M)).astype(np.int32), rng.standard_normal((B, M)).astype(f32),
             rng.integers(0, M, B).astype(np.int32), rng.integers(0, 50, B).astype(np.int32)]
    rows = np.array([B - 1, 0, B + 5, 1, -1], np.int32)              # B + 5 and -1: outside, skipped
    _, src, _, _, _ = _state_case(5, V, 7 + B)
    src = list(src) + [rng.integers(1, 50, 5).astype(np.int32)]
    src[1][:] = [1, 0, 1, 1, 1]
    src[4][:] = [M if V > M else 9, 0, 5, 1, 3]
    want = [a.copy() for a in state]
    edit_reset_np(want, rows, src)
    if B > 3:                                                        # (a row not listed keeps its state)
        assert all(np.array_equal(w[2:B - 1], a[2:B - 1]) for w, a in zip(want, state))
    D, S, R = [hip.from_numpy(a) for a in state], [hip.from_numpy(a) for a in src], hip.from_numpy(rows)
    L.call("pdne_logit_edit_reset", *(a._ptr for a in D), B, V, R._ptr, 5, *(a._ptr for a in S), hip.stream())
    for d, w in zip(D, want):
        assert np.array_equal(d.get().view(np.int32), w.view(np.int32))
    # without sources: the allowed sets off and the tables empty, bits and entries as they were
    want2 = [a.copy() for a in want]
    edit_reset_np(want2, rows[:2], (None, None, None, None, None, src[5][:2]))
    L.call("pdne_logit_edit_reset", *(a._ptr for a in D), B, V, R._ptr, 2, None, None, None, None, None, S[5]._ptr,
           hip.stream())
    for d, w in zip(D, want2):
        assert np.array_equal(d.get().view(np.int32), w.view(np.int32))
    assert want2[1][0] == 0 and want2[4][B - 1] == 0


# -- end to end ----------------------------------------------------------------------------------------------------
VOCAB = 2500                                                         # three vocabulary chunks, the last one partial


def _model(dev, B):
    np.random.seed(8)
    m = Llama(VOCAB, 96, 2, 128, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(VOCAB, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to(dev) if dev != "cpu" else m


def _run(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn()
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _prompts(N, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, VOCAB, 1 + (7 * r) % 11) for r in range(N)]


def _edits(N, seed):
    """Every request different: a bias (bans, a push, shifts across the three chunks), an allowed set, both or neither."""
    rng = np.random.default_rng(1000 + seed)
    bias, allow = [], []
    for r in range(N):
        ids = rng.permutation(VOCAB)[:40 + r]
        b = {int(t): float(v) for t, v in zip(ids, rng.standard_normal(ids.size) * 2)}
        for t in ids[:12]:
            b[int(t)] = -INF
        b[int(ids[12])] = 4.0
        a = np.sort(rng.permutation(VOCAB)[:300 + 5 * r])
        bias.append(b if r % 4 in (0, 2) else None)
        allow.append(a if r % 4 in (1, 2) else None)
    return dict(logit_bias=bias, allowed_token_ids=allow)


def _steps(it):
    return np.stack([t.numpy().reshape(-1) for t in it], 1)


def _reference(prompts, n, ed, stops=(), m=0, pen=None, **kw):
    """generate_ragged on `cpu` with every step's EDITED logits (the statements on the recorded projections)."""
    mod = _model("cpu", len(prompts))
    raw = []
    fwd = mod.lm_head.forward

    def rec(x):
        y = fwd(x)
        raw.append(np.asarray(y.numpy(), np.float32)[:, -1, :])
        return y
    mod.lm_head.forward = rec
    try:
        toks = _run(mod, lambda: _steps(mod.generate_ragged(prompts, n, stop_ids=stops, min_new_tokens=m, **kw, **ed,
                                                            **(pen or {}))))
    finally:
        del mod.lm_head.forward
    spec = E.check_args(ed["logit_bias"], ed["allowed_token_ids"], m, VOCAB, len(prompts), stops)
    seen = penalties.seen_rows(prompts, VOCAB)
    R = range(len(prompts))
    logits = []
    for s, z in enumerate(raw):
        if pen:
            c = np.zeros((len(prompts), VOCAB), np.int64)
            for r in R:
                prev = toks[r, :s]
                np.add.at(c[r], prev[prev >= 0], 1)
            z = penalties.penalize(z, c, seen, *penalties.check_args(**pen))
        logits.append(E.apply(z, spec.allow_rows(R), spec.bias_rows(R), np.full(len(prompts), s), m, stops))
    return toks, logits


def _margin(z, pos, r, kw):
    if kw:
        return margin(z, pos, r, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw["seed"])
    srt = np.sort(z.astype(np.float64))
    return srt[-1] - srt[-2]


def _near_tie_rows(ref, logits, prompts, budgets, kw):
    """Rows of the CPU reference with a step at a float64 decision margin below 1e-5 (inside their budget)."""
    rows = set()
    for r in range(ref.shape[0]):
        for s in range(min(ref.shape[1], budgets[r])):
            if ref[r, s] < 0:
                break
            if _margin(logits[s][r], len(prompts[r]) + s, r, kw) < 1e-5:
                rows.add(r)
    return rows


def _check(got, ref, logits, prompts, budgets, stops, kw):
    """Tokens equal the reference's up to the first step whose float64 decision margin is below 1e-5 -- a condition, not a
    tolerance: at most 1 row in 20 may use it, and the CPU reference alone has no more such rows."""
    assert len(_near_tie_rows(ref, logits, prompts, budgets, kw)) <= len(got) // 20
    escaped = 0
    for r, g in enumerate(got):
        g = np.asarray(g)
        w = ref[r, :budgets[r]].tolist()
        hit = next((i for i, t in enumerate(w) if t in stops or t < 0), None)
        w = np.array(w if hit is None else w[:hit + 1])
        w = w[w >= 0]
        if np.array_equal(g, w):
            continue
        n = min(len(g), len(w))
        bad = np.flatnonzero(g[:n] != w[:n])
        assert bad.size, (r, g, w)
        s = int(bad[0])
        mg = _margin(logits[s][r], len(prompts[r]) + s, r, kw)
        assert mg < 1e-5, (r, s, mg)
        escaped += 1
    assert escaped <= len(got) // 20, escaped


def _check_properties(got, ed, stops=(), m=0):
    for r, toks in enumerate(got):
        toks = [int(t) for t in toks if t >= 0]
        b, a = ed["logit_bias"][r], ed["allowed_token_ids"][r]
        if b is not None:
            assert not {t for t, v in b.items() if v == -INF} & set(toks), r
        if a is not None:
            assert set(toks) <= set(a.tolist()), r
        assert not set(toks[:m]) & set(stops), r


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [1, 8, 16, 64])
def test_generate_ragged_and_generate(hip, B, kw):
    Graph.clear()
    prompts = _prompts(B, B)
    ed = _edits(B, B)
    n = 10
    ref, logits = _reference(prompts, n, ed, **kw)
    m = _model("hip:0", B)
    got = _run(m, lambda: _steps(m.generate_ragged(prompts, n, **kw, **ed)))
    _check(got, ref, logits, prompts, [n] * B, set(), kw)
    _check_properties(got, ed)
    assert m._decode_st["edit"] and m._decode_st["ok"] and m._decode_st["wide"] == (B > 8)
    # a stop id the reference picks at its third step, held back until 6 tokens are out
    stops = {int(ref[0, 2])}
    ref_s, logits_s = _reference(prompts, n, ed, stops, 6, **kw)
    m = _model("hip:0", B)                           # (a fresh cache: a step reads the slot after its prompt unwritten)
    got = _run(m, lambda: _steps(m.generate_ragged(prompts, n, stop_ids=stops, min_new_tokens=6, **kw, **ed)))
    _check([r[r >= 0] for r in got], ref_s, logits_s, prompts, [n] * B, stops, kw)
    _check_properties(got, ed, stops, 6)
    assert (got[0, :6] >= 0).all()
    # generate: equal lengths, the rectangular step
    ids = np.stack([np.resize(p, 6) for p in prompts])
    ref, logits = _reference(list(ids), n, ed, **kw)
    m = _model("hip:0", B)
    got = _run(m, lambda: _steps(m.generate(ids, 6 + n, **kw, **ed)))
    _check(got, ref, logits, list(ids), [n] * B, set(), kw)
    _check_properties(got, ed)


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("slots,chunk", [(8, None), (8, 6), (16, 8), (64, None)])
def test_serve(hip, slots, chunk, kw):
    Graph.clear()
    N = slots + 6
    prompts = _prompts(N, slots + (chunk or 0))
    ed = _edits(N, slots)
    budgets = [2 + (5 * r) % 13 for r in range(N)]
    ref, logits = _reference(prompts, int(max(budgets)), ed, **kw)
    m = _model("hip:0", N)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=slots, prefill_chunk=chunk, **kw, **ed))
    _check(got, ref, logits, prompts, budgets, set(), kw)
    _check_properties(got, ed)
    assert m._decode_st["edit"] and m._decode_st["ok"]


def test_with_penalties_and_logprobs(hip):
    """Penalties, edits and logprobs together, ragged and served (chunked, with the prefix cache): the edit kernel runs
    behind the penalty kernel and hands the tick its candidates; a banned token's log-probability is -inf."""
    Graph.clear()
    B, n = 8, 12
    prompts = _prompts(B, 5)
    ed = _edits(B, 5)
    ed["allowed_token_ids"][1], ed["logit_bias"][1] = np.array([11, 2040]), None
    ref, logits = _reference(prompts, n, ed, pen=PEN)
    m = _model("hip:0", B)
    steps = _run(m, lambda: [(t.numpy().reshape(-1).copy(), lp) for t, lp in
                             m.generate_ragged(prompts, n, logprobs=3, **PEN, **ed)])
    got = np.stack([s[0] for s in steps], 1)
    _check(got, ref, logits, prompts, [n] * B, set(), {})
    _check_properties(got, ed)
    st = m._decode_st
    assert st["edit"] and st["pen"] and st["lp_n"] == 3 and st["ok"]
    top = np.stack([s[1].top_logprobs for s in steps], 1)            # (B, steps, 3)
    assert (top[1, :, 2] == -INF).all() and np.isfinite(top[1, :, :2]).all()
    assert set(got[1].tolist()) <= {11, 2040}
    budgets = [2 + (5 * r) % 11 for r in range(B)]
    m = _model("hip:0", B)
    out = _run(m, lambda: m.serve_all(prompts, budgets, slots=3, prefill_chunk=4, prefix_cache=True, logprobs=3, **PEN,
                                      **ed))
    _check([o[0] for o in out], ref, logits, prompts, budgets, set(), {})
    assert (out[1][1].top_logprobs[:, 2] == -INF).all()


def test_plan_after_graph_replayed_run(hip, monkeypatch):
    """A graph-replayed run: the plan holds graphs and the edit state, and the replays do not pass through the entry (its
    counter stays below the step count); launch by launch the same tokens, with one launch of the edit kernel per step
    (plus the reset and the prompt pass)."""
    Graph.clear()
    n = 12
    for B in (4, 12):
        prompts = _prompts(B, 40 + B)
        ed = _edits(B, 40 + B)
        m = _model("hip:0", B)
        _counters()
        got = _run(m, lambda: _steps(m.generate_ragged(prompts, n, **ed)))
        c = _counters()
        st = m._decode_st
        assert st["edit"] and st["graphs"] and st["key"][-1] == "edit" and 0 < c[48] < n and c[35] == 0
        assert st["edit_start"].get().tolist() == [p.size for p in prompts]
        bits, on, ids, vals, cnt = E.check_args(V=VOCAB, n=B, **ed).packed(range(B))
        assert np.array_equal(st["edit_allow_on"].get(), on) and np.array_equal(st["edit_bias_n"].get(), cnt)
        assert np.array_equal(st["edit_allow"].get()[on > 0], bits[on > 0])
        monkeypatch.setattr(Llama, "graph_decode", False)
        m = _model("hip:0", B)
        _counters()
        again = _run(m, lambda: _steps(m.generate_ragged(prompts, n, **ed)))
        c = _counters()
        monkeypatch.setattr(Llama, "graph_decode", True)
        assert np.array_equal(got, again) and not m._decode_st["graphs"]
        assert c[48] == (n - 1) + 2                                  # one per decode step, the reset, the prompt pass
        _check_properties(got, ed)


def test_defaults_keep_the_plan_key_and_the_counters(hip):
    Graph.clear()
    prompts = _prompts(5, 3)
    m0, m1 = _model("hip:0", 5), _model("hip:0", 5)
    _counters()
    base = _run(m0, lambda: _steps(m0.generate_ragged(prompts, 10, stop_ids=[7])))
    c0 = _counters()
    Graph.clear()
    again = _run(m1, lambda: _steps(m1.generate_ragged(prompts, 10, stop_ids=[7], logit_bias=None, allowed_token_ids=None,
                                                       min_new_tokens=0)))
    c1 = _counters()
    k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
    assert np.array_equal(base, again) and c0 == c1 and c0[48] == 0
    assert len(k0) == len(k1) == 11 and k0[:5] == k1[:5] and k0[6:] == k1[6:]      # (index 5: the weights' addresses)
    assert m1._decode_st["edit"] is False and "edit_allow" not in m1._decode_st and not m1._decode_st["full"]
