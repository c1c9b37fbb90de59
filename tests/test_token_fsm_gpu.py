"""token_fsm on a real MI355X: the entries of csrc/token_fsm.hip bit for bit against the statement
(tests/abi_emulator/_fsm.py over llm/token_fsm.py), a captured step replayed 50 times with resets in between against the
host walk (the hand-off of a row's state between its chunk workgroups), and `generate`, `generate_ragged` and `serve` end
to end against the `cpu` device under the first-difference margin rule of tests/test_penalties_gpu.py, on the narrow (<= 8
rows) and the wide step.  Every GPU sequence is walked through its machine in plain Python: acceptance has no tolerance."""
import ctypes

import numpy as np
import pytest

from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import token_fsm as F
from pydynet_amd.llm.token_fsm import TokenFSM
from tests.abi_emulator._fsm import fsm_chunks as chunks, fsm_np, fsm_reset_np
from tests.test_logit_edits_gpu import SAMPLED, VOCAB, _check, _model, _prompts, _run, _steps

pytestmark = pytest.mark.gpu
f32 = np.float32
INF = np.inf
NSLOT = 53


def _counters():
    buf = (ctypes.c_int64 * NSLOT)()
    _lib.lib().call("pdn_kernel_counters", buf, NSLOT, 1)
    return [int(v) for v in buf]


_MACHINES = {}


def _machine(V):
    """Six kinds of state: 0 a single allowed token; 1 a default and nothing else; 2 a default with explicit overrides;
    3 edges on the first and last token of the first, second and last chunks and of the row; 4 a random half of the
    vocabulary (a long sorted list to search); 5 a default, entered from 4."""
    if V not in _MACHINES:
        rng = np.random.default_rng(V)
        edge = sorted({t % V for t in (0, 1023, 1024, V - 1025, V - 1024, V - 1)})
        half = np.flatnonzero(rng.random(V) < 0.5)
        _MACHINES[V] = (TokenFSM([{V - 2: 3}, {}, {5: 0, 1030 % V: 3, V - 1: 4}, {t: (0, 2, 4)[i % 3] for i, t in enumerate(edge)},
                                  {int(t): int(4 + (t % 2)) for t in half}, {}], 0, [-1, 2, 1, -1, -1, 4]), edge, half)
    return _MACHINES[V]


def _step_case(B, V, seed):
    """Logit rows with zeros and infinities, and rows whose word states cycle through off (-1) and the six kinds of state,
    at g = 0 (the start state, whatever the word holds), g > 0 fed a token with an edge, g > 0 fed one without (the default,
    or the state kept), and with the word already at this position; every seventh row at position -1."""
    rng = np.random.default_rng(seed)
    fsm, edge, half = _machine(V)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    z[:, ::97] = 0.0
    z[:, 5::131] = -0.0
    z[:, 7::101] = -INF
    z[:, 11::211] = INF
    b = np.arange(B)
    ws = (b + seed) % 7 - 1                                          # the word's state
    s0 = (3 * b + seed + 2) % 7 - 1                                  # the start state
    kind = (b // 7 + b + seed) % 4                                   # 0: g = 0; 1: an edge; 2: no edge; 3: word at pos
    pos = rng.integers(3, 60, B).astype(np.int32)
    start = np.where(kind == 0, pos + (b % 2), pos - 1 - b % 3).astype(np.int32)    # (g = 0 or below; else g = 1 .. 3)
    tag = np.where(kind == 3, pos, pos - 1 - (b % 2) * 5).astype(np.int32)           # (an older tag, not always pos - 1)
    with_edge = {-1: 9, 0: V - 2, 1: 9, 2: 1030 % V, 3: edge[-1], 4: int(half[-1]), 5: 9}
    without = {-1: 9, 0: 3, 1: 9, 2: 6, 3: 2 % V if 2 % V not in edge else 3, 4: int(np.setdiff1d(np.arange(64), half)[0]), 5: 9}
    ids = np.array([with_edge[int(s)] if k == 1 else without[int(s)] for s, k in zip(ws, kind)], np.int64)
    pos[3::7] = -1                                                   # skipped rows stay untouched
    return z, fsm, F.pair(ws, tag), s0.astype(np.int32), start, ids, pos


def _tables(hip, fsm):
    S_cap, E_cap = F.capacity(fsm.S, 64), F.capacity(fsm.E, 1024)
    host = F.padded(fsm, S_cap, E_cap)
    return host, [hip.from_numpy(a) for a in host], S_cap, E_cap


@pytest.mark.parametrize("V", [32000, 1001])
@pytest.mark.parametrize("B", [1, 8, 64, 256])
def test_fsm_entries_bit_equal(hip, B, V):
    L = _lib.lib()
    z, fsm, word, s0, start, ids, pos = _step_case(B, V, B + V)
    n = L.query("pdnf_fsm_chunks", V)
    assert n == chunks(V)
    host, T, S_cap, E_cap = _tables(hip, fsm)
    # the step's form: the state from the word, the start state and the fed token; candidates
    want, w_word = z.copy(), word.copy()
    live, cv, ci = fsm_np(want, fsm, word=w_word, start_state=s0, start=start, ids=ids, pos=pos)
    assert np.array_equal(live, pos >= 0) and not np.isnan(want).any()
    assert np.array_equal(w_word[~live], word[~live]) and (B < 8 or not np.array_equal(w_word, word))
    Z, W, S0, ST, I, P = (hip.from_numpy(a) for a in (z, word, s0, start, ids.reshape(B, 1), pos))
    CV, CI = hip.from_numpy(np.full((B, n), 7.0, f32)), hip.from_numpy(np.full((B, n), -7, np.int32))
    L.call("pdnf_fsm_step_f32", Z._ptr, V, B, V, *(a._ptr for a in T), S_cap, E_cap, W._ptr, S0._ptr, ST._ptr, I._ptr,
           P._ptr, 1, CV._ptr, CI._ptr, hip.stream())
    got = Z.get()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(got[~live].view(np.int32), z[~live].view(np.int32))
    assert np.array_equal(W.get(), w_word)                           # rows at -1: the word kept
    assert np.array_equal(CV.get()[live].view(np.int32), cv[live].view(np.int32))
    assert np.array_equal(CI.get()[live], ci[live])
    assert (CV.get()[~live] == 7.0).all() and (CI.get()[~live] == -7).all()
    for a, d in zip(host, T):                                        # the tables are only read
        assert np.array_equal(d.get(), a)
    assert np.array_equal(S0.get(), s0) and np.array_equal(ST.get(), start) and np.array_equal(I.get().reshape(-1), ids)
    # the same launch again: every word is at its position now and is taken as it is
    Z = hip.from_numpy(z)
    L.call("pdnf_fsm_step_f32", Z._ptr, V, B, V, *(a._ptr for a in T), S_cap, E_cap, W._ptr, S0._ptr, ST._ptr, I._ptr,
           P._ptr, 1, None, None, hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32)) and np.array_equal(W.get(), w_word)
    # the rows form: explicit states, read only, with and without the skip marks and the candidates
    # (-1 .. 6 and 70: state 6 is one of the capacity's states behind the machine's, without an edge or a default: it
    #  allows nothing; state 70 lies outside the tables: no mask)
    states = ((np.arange(B) * 5 + 3) % 9 - 1).astype(np.int32)
    states[states == 7] = 70
    full = F.Tables(*host)
    want = z.copy()
    _, cv, ci = fsm_np(want, full, states=states, pos=pos)
    assert B < 64 or ((want[(states == 6) & live] == -INF).all() and np.array_equal(want[states == 70], z[states == 70]))
    Z, D = hip.from_numpy(z), hip.from_numpy(states)
    L.call("pdnf_fsm_rows_f32", Z._ptr, V, B, V, T[0]._ptr, T[1]._ptr, T[3]._ptr, S_cap, E_cap, D._ptr, P._ptr, CV._ptr,
           CI._ptr, hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32)) and np.array_equal(D.get(), states)
    assert np.array_equal(CV.get()[live].view(np.int32), cv[live].view(np.int32)) and np.array_equal(CI.get()[live], ci[live])
    want = z.copy()
    fsm_np(want, full, states=states)
    Z = hip.from_numpy(z)
    L.call("pdnf_fsm_rows_f32", Z._ptr, V, B, V, T[0]._ptr, T[1]._ptr, T[3]._ptr, S_cap, E_cap, D._ptr, None, None, None,
           hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32))


def test_step_entry_row_stride_and_shared_position(hip):
    """A logits row stride wider than V with the tail untouched, and the rectangular form (pos_per_row = 0: every row at
    pos[0]); a chunk of nothing but NaN yields (NaN, its first index), elsewhere a NaN never wins; a banned NaN is -inf."""
    L = _lib.lib()
    B, V, rs = 7, 3001, 3072
    z, fsm, word, s0, start, ids, _ = _step_case(B, V, 5)
    pos = np.array([30], np.int32)
    start = np.array([30, 29, 28, 12, 29, 31, 27], np.int32)
    word = F.pair(F.unpair(word)[0], np.array([29, 29, 30, 30, 11, 29, 26]))
    s0[3], word[3] = 1, F.pair(1, 30)                                # (row 3 in a default state: its NaN chunk stays)
    z[3, 1024:2048] = np.nan
    z[4, 2050] = np.nan
    z[5, 5] = np.nan                                                 # (row 5, at g < 0, starts in state 0: banned)
    zz = np.full((B, rs), 3.0, f32)
    zz[:, :V] = z
    want, w_word = z.copy(), word.copy()
    _, cv, ci = fsm_np(want, fsm, word=w_word, start_state=s0, start=start, ids=ids, pos=np.full(B, 30))
    assert np.isnan(cv[3, 1]) and ci[3, 1] == 1024 and np.isnan(want[3, 1024:2048]).all() and np.isnan(want[4, 2050])
    assert want[5, 5] == -INF and np.isinf(want[5]).sum() == V - 1
    host, T, S_cap, E_cap = _tables(hip, fsm)
    n = chunks(V)
    Z, W, S0, ST, I, P = (hip.from_numpy(a) for a in (zz, word, s0, start, ids.reshape(B, 1), pos))
    CV, CI = hip.from_numpy(np.zeros((B, n), f32)), hip.from_numpy(np.zeros((B, n), np.int32))
    L.call("pdnf_fsm_step_f32", Z._ptr, rs, B, V, *(a._ptr for a in T), S_cap, E_cap, W._ptr, S0._ptr, ST._ptr, I._ptr,
           P._ptr, 0, CV._ptr, CI._ptr, hip.stream())
    got = Z.get()
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got[:, :V]), ~ok) and np.array_equal(got[:, :V][ok].view(np.int32), want[ok].view(np.int32))
    assert (got[:, V:] == 3.0).all() and np.array_equal(W.get(), w_word)
    assert np.array_equal(CI.get(), ci) and np.array_equal(np.isnan(CV.get()), np.isnan(cv))
    assert np.array_equal(CV.get()[~np.isnan(cv)].view(np.int32), cv[~np.isnan(cv)].view(np.int32))


@pytest.mark.parametrize("B", [3, 700])
def test_reset_entry(hip, B):
    L = _lib.lib()
    rng = np.random.default_rng(B)
    state = [rng.integers(-2 ** 62, 2 ** 62, B), rng.integers(-1, 50, B).astype(np.int32),
             rng.integers(0, 50, B).astype(np.int32)]
    R = 5 if B == 3 else 300                                         # (300 rows: more than one workgroup)
    rows = rng.permutation(B)[:R].astype(np.int32) if B > 3 else np.array([B - 1, 0, B + 5, 1, -1], np.int32)
    if B > 3:
        rows[7], rows[260] = B + 5, -1                               # outside: skipped
    src = (rng.integers(-1, 60000, R).astype(np.int32), rng.integers(1, 2000, R).astype(np.int32))
    want = [a.copy() for a in state]
    fsm_reset_np(want, rows, src)
    listed = np.isin(np.arange(B), rows)
    assert all(np.array_equal(w[~listed], a[~listed]) for w, a in zip(want, state)) and (B == 3 or (~listed).sum() > 300)
    D, S, RW = [hip.from_numpy(a) for a in state], [hip.from_numpy(a) for a in src], hip.from_numpy(rows)
    L.call("pdnf_fsm_reset", *(a._ptr for a in D), B, RW._ptr, R, S[0]._ptr, S[1]._ptr, hip.stream())
    for d, w in zip(D, want):
        assert np.array_equal(d.get(), w)
    st, tag = F.unpair(D[0].get()[listed])
    assert np.array_equal(st, want[1][listed]) and np.array_equal(tag, want[2][listed])


def test_replayed_step_hands_the_state_on(hip):
    """A captured step -- the FSM kernel over 64 rows x 32 chunks -- replayed 50 times; between the replays the host feeds
    new tokens, advances the positions and resets some rows.  After every replay the words, the masked rows and the
    candidates equal the host walk: whichever word a chunk workgroup read, it arrived at the state chunk 0 stored."""
    L = _lib.lib()
    B, V = 64, 32000
    rng = np.random.default_rng(50)
    fsm, edge, half = _machine(V)
    host, T, S_cap, E_cap = _tables(hip, fsm)
    n = chunks(V)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    s0 = (np.arange(B) % 7 - 1).astype(np.int32)
    start = rng.integers(1, 9, B).astype(np.int32)
    pos = start.copy()
    pos[5::11] = -1                                                  # rows that never run
    word = F.pair(np.full(B, -1), np.zeros(B))
    Z0, Z, W, S0, ST = (hip.from_numpy(a) for a in (z, z, word, s0, start))
    I, P = hip.from_numpy(np.zeros((B, 1), np.int64)), hip.from_numpy(pos)
    CV, CI = hip.from_numpy(np.zeros((B, n), f32)), hip.from_numpy(np.zeros((B, n), np.int32))
    rows = np.arange(B, dtype=np.int32)
    RW, RS, RL = hip.from_numpy(rows), hip.from_numpy(s0), hip.from_numpy(start)
    L.call("pdnf_fsm_reset", W._ptr, S0._ptr, ST._ptr, B, RW._ptr, B, RS._ptr, RL._ptr, hip.stream())
    h_state = [word.copy(), s0.copy(), start.copy()]
    fsm_reset_np(h_state, rows, (s0, start))

    def launches():
        L.call("pdnf_fsm_step_f32", Z._ptr, V, B, V, *(a._ptr for a in T), S_cap, E_cap, W._ptr, S0._ptr, ST._ptr, I._ptr,
               P._ptr, 1, CV._ptr, CI._ptr, hip.stream())
    g = hip.Graph()
    g.capture(launches)                                              # (two real runs at g = 0: the start states)
    ids = np.zeros(B, np.int64)
    try:
        for it in range(50):
            if it:
                # the tokens fed: one of the state's own edges, or any token (its default, or none: the state is kept)
                cur = F.unpair(h_state[0])[0]
                for b in range(B):
                    lo, hi = (fsm.offsets[cur[b]], fsm.offsets[cur[b] + 1]) if 0 <= cur[b] < fsm.S else (0, 0)
                    ids[b] = fsm.tokens[rng.integers(lo, hi)] if hi > lo and rng.random() < 0.7 else rng.integers(0, V)
                pos = np.where(pos >= 0, pos + 1, -1).astype(np.int32)
                I[...] = ids.reshape(B, 1)
                P[...] = pos
            if it % 6 == 4:                                          # some rows take a new request
                r = rng.permutation(B)[:9].astype(np.int32)
                r = r[pos[r] >= 0]
                ns, nl = rng.integers(-1, 6, r.size).astype(np.int32), (pos[r] + rng.integers(0, 2, r.size)).astype(np.int32)
                RW, RS, RL = hip.from_numpy(r), hip.from_numpy(ns), hip.from_numpy(nl)
                L.call("pdnf_fsm_reset", W._ptr, S0._ptr, ST._ptr, B, RW._ptr, int(r.size), RS._ptr, RL._ptr, hip.stream())
                fsm_reset_np(h_state, r, (ns, nl))
            Z[...] = Z0
            g.replay()
            want = z.copy()
            live, cv, ci = fsm_np(want, fsm, word=h_state[0], start_state=h_state[1], start=h_state[2], ids=ids, pos=pos)
            assert np.array_equal(W.get(), h_state[0]), it
            assert np.array_equal(Z.get().view(np.int32), want.view(np.int32)), it
            assert np.array_equal(CI.get()[live], ci[live]) and np.array_equal(CV.get()[live].view(np.int32),
                                                                              cv[live].view(np.int32)), it
    finally:
        g.destroy()
    seen = set(F.unpair(h_state[0])[0].tolist())
    assert len(seen) >= 4                                            # (the walk visited the machine, not one state)
    for a, d in zip(host, T):
        assert np.array_equal(d.get(), a)


# -- end to end ----------------------------------------------------------------------------------------------------
END = VOCAB - 1


def _seqs(seed):
    """16 choices of 1 .. 4 tokens over the three vocabulary chunks, one a proper prefix of another."""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, VOCAB - 1, 1 + i % 4).tolist() for i in range(16)]
    out[0] = out[3][:2]
    return out


SEQS = _seqs(77)
CHOICE = TokenFSM.from_sequences(SEQS, END)
FREE = TokenFSM.free_until(1500, TokenFSM.from_sequences([[3, 2047], [2048]], END))


def _machines(N):
    return [(CHOICE, FREE, None, CHOICE)[r % 4] for r in range(N)]


def _walk(fsm, toks):
    """A plain-Python walk of `fsm` over `toks`: the states before each token, or None when a token is not allowed."""
    s, out = fsm.start, []
    for t in toks:
        out.append(s)
        edges = {int(fsm.tokens[j]): int(fsm.next[j]) for j in range(int(fsm.offsets[s]), int(fsm.offsets[s + 1]))}
        if t in edges:
            s = edges[t]
        elif fsm.dflt[s] >= 0:
            s = int(fsm.dflt[s])
        else:
            return None
    return out + [s]


def _check_accepted(got, fsms, stopped=True):
    for r, (toks, f) in enumerate(zip(got, fsms)):
        toks = [int(t) for t in toks if t >= 0]
        if f is None:
            continue
        assert _walk(f, toks) is not None, (r, toks)
        if f is CHOICE:                                              # one of the choices, then the end
            body = toks[:toks.index(END)] if END in toks else toks
            assert any(body == c[:len(body)] for c in SEQS) and (END not in toks or body in SEQS), (r, toks)
            assert END in toks or len(toks) < 5 or not stopped, (r, toks)


def _reference(prompts, n, fsms, stops=(), **kw):
    """generate_ragged on `cpu` with every step's MASKED logits (the statement on the recorded projections, each row in
    the state a plain walk of its tokens so far ends in)."""
    mod = _model("cpu", len(prompts))
    raw = []
    fwd = mod.lm_head.forward

    def rec(x):
        y = fwd(x)
        raw.append(np.asarray(y.numpy(), np.float32)[:, -1, :])
        return y
    mod.lm_head.forward = rec
    try:
        toks = _run(mod, lambda: _steps(mod.generate_ragged(prompts, n, stop_ids=stops, token_fsm=fsms, **kw)))
    finally:
        del mod.lm_head.forward
    logits = []
    for s, z in enumerate(raw):
        z = z.copy()
        for r, f in enumerate(fsms):
            prev = toks[r, :s]
            if f is not None and (prev >= 0).all():
                z[r] = F.apply(z[r:r + 1], f, [_walk(f, prev.tolist())[-1]])[0]
        logits.append(z)
    return toks, logits


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [1, 8, 16, 64])
def test_generate_ragged_and_generate(hip, B, kw):
    Graph.clear()
    prompts = _prompts(B, B)
    fsms = _machines(B)
    n = 10
    stops = {END}
    ref, logits = _reference(prompts, n, fsms, stops, **kw)
    m = _model("hip:0", B)
    got = _run(m, lambda: _steps(m.generate_ragged(prompts, n, stop_ids=stops, token_fsm=fsms, **kw)))
    _check([r[r >= 0] for r in got], ref, logits, prompts, [n] * B, stops, kw)
    _check_accepted(got, fsms)
    st = m._decode_st
    assert st["fsm"] and st["ok"] and st["wide"] == (B > 8)
    # generate: equal lengths, the rectangular step, no stop ids: the end token repeats
    ids = np.stack([np.resize(p, 6) for p in prompts])
    ref, logits = _reference(list(ids), n, fsms, **kw)
    m = _model("hip:0", B)
    got = _run(m, lambda: _steps(m.generate(ids, 6 + n, token_fsm=fsms, **kw)))
    _check(got, ref, logits, list(ids), [n] * B, set(), kw)
    _check_accepted(got, fsms)
    assert (got[0, 5:] == END).all()                                 # (a choice of at most 4 tokens, then the end for good)
    assert st["graphs"] and m._decode_st["graphs"] and m._decode_st["fsm"]


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("slots,chunk", [(8, None), (8, 6), (16, 8), (64, None)])
def test_serve(hip, slots, chunk, kw):
    Graph.clear()
    N = slots + 6
    prompts = _prompts(N, slots + (chunk or 0))
    fsms = _machines(N)
    budgets = [2 + (5 * r) % 13 for r in range(N)]
    stops = {END}
    ref, logits = _reference(prompts, int(max(budgets)), fsms, stops, **kw)
    m = _model("hip:0", N)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=slots, prefill_chunk=chunk, stop_ids=stops, token_fsm=fsms,
                                      **kw))
    _check(got, ref, logits, prompts, budgets, stops, kw)
    _check_accepted(got, fsms, stopped=False)
    assert m._decode_st["fsm"] and m._decode_st["ok"]


def test_plan_and_counters(hip, monkeypatch):
    """A graph-replayed run holds graphs and the FSM state, and its replays do not pass through the entry; launch by launch
    the same tokens with one launch of the FSM kernel per step (plus the reset and the prompt pass).  With token_fsm=None
    the plan key and the counters are those of a run without the keyword."""
    from pydynet_amd.llm.llama import Llama
    Graph.clear()
    n, B = 12, 4
    prompts = _prompts(B, 44)
    fsms = _machines(B)
    m = _model("hip:0", B)
    _counters()
    got = _run(m, lambda: _steps(m.generate_ragged(prompts, n, token_fsm=fsms)))
    c = _counters()
    st = m._decode_st
    spec = F.check_args(fsms, VOCAB, B)
    assert st["fsm"] and st["graphs"] and st["key"][-3:] == ("fsm",) + spec.caps and 0 < c[52] < n and c[48] == 0
    assert st["fsm_start"].get().tolist() == [p.size for p in prompts]
    assert np.array_equal(st["fsm_start_state"].get(), spec.starts)
    for name, a in zip(("fsm_off", "fsm_tok", "fsm_next", "fsm_dflt"), F.padded(spec.tables, *spec.caps)):
        assert np.array_equal(st[name].get(), a)
    states, tags = F.unpair(st["fsm_state"].get())                   # every row's word: its last step's position and state
    for r, f in enumerate(fsms):
        assert tags[r] == prompts[r].size + n - 1
        assert states[r] == (-1 if f is None else spec.starts[r] - f.start + _walk(f, got[r, :n - 1].tolist())[-1])
    monkeypatch.setattr(Llama, "graph_decode", False)
    m = _model("hip:0", B)
    _counters()
    again = _run(m, lambda: _steps(m.generate_ragged(prompts, n, token_fsm=fsms)))
    c = _counters()
    monkeypatch.setattr(Llama, "graph_decode", True)
    assert np.array_equal(got, again) and not m._decode_st["graphs"] and c[52] == (n - 1) + 2
    _check_accepted(got, fsms, stopped=False)
    Graph.clear()
    m0, m1 = _model("hip:0", B), _model("hip:0", B)
    _counters()
    base = _run(m0, lambda: _steps(m0.generate_ragged(prompts, 10, stop_ids=[7])))
    c0 = _counters()
    Graph.clear()
    again = _run(m1, lambda: _steps(m1.generate_ragged(prompts, 10, stop_ids=[7], token_fsm=None)))
    c1 = _counters()
    k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
    assert np.array_equal(base, again) and c0 == c1 and c0[52] == 0
    assert len(k0) == len(k1) == 11 and k0[:5] == k1[:5] and k0[6:] == k1[6:]      # (index 5: the weights' addresses)
    assert m1._decode_st["fsm"] is False and "fsm_off" not in m1._decode_st and not m1._decode_st["full"]
