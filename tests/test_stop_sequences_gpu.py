"""stop_sequences on a real MI355X: the entries of csrc/stop_seq.hip exact-equal to the statement
(tests/abi_emulator/_stopseq.py over llm/stop_sequences.py), a captured step replayed with a sequence completing on the third
replay, and `generate_ragged` / `serve` end to end on the narrow (<= 8 rows), the wide and the mixed step: a request's
output with stop sequences is its output without them on the same device, truncated at the match -- no tolerance."""
import ctypes

import numpy as np
import pytest

from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import stop_sequences as SS
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator._stopseq import stop_reset_np, stop_step_np
from tests.test_logit_edits_gpu import SAMPLED, VOCAB, _model, _prompts, _run, _steps
from tests.test_stop_sequences import served_state_follows

pytestmark = pytest.mark.gpu
NSLOT = 54
CAPS = (16, 64, 256)
# set 0: empty; 1: 16 sequences of length 1 (every lane that looks); 2: lengths 16 and 1; 3: one a suffix of another
SETS = [[], [[t] for t in range(100, 116)], [list(range(200, 216)), [7]], [[5, 6, 7], [6, 7], [9, 9, 8]]]
MIN_NEW = 2


def _counters():
    buf = (ctypes.c_int64 * NSLOT)()
    _lib.lib().call("pdn_kernel_counters", buf, NSLOT, 1)
    return [int(v) for v in buf]


def _step_case(B, seed):
    """Rows cycling through: a match (every sequence of every set in turn, set 1 through all 16 lanes), a near miss, a match
    at g <= min_new (ignored), the empty set, position -1 and set -1 (both untouched)."""
    rng = np.random.default_rng(seed)
    tables = SS.packed(SETS)
    flat_seqs = [(s, q) for s, qs in enumerate(SETS) for q in qs]
    ids = rng.integers(300, 400, B).astype(np.int64)
    sets = np.zeros(B, np.int32)
    start = rng.integers(1, 50, B).astype(np.int32)
    tail = rng.integers(300, 400, (B, 16)).astype(np.int32)
    pos = np.zeros(B, np.int32)
    kinds = (np.arange(B) + 2) % 6
    for b in range(B):
        s, q = flat_seqs[(b // 6 * 5 + b) % len(flat_seqs)]
        k = kinds[b]
        g = len(q) + MIN_NEW + int(rng.integers(0, 40)) if k != 4 else len(q)
        if k == 4 and len(q) > MIN_NEW:
            k = 2                                                     # (longer than min_new: a plain match at g = l)
        sets[b] = s
        for j in range(1, len(q)):
            tail[b, (g - j) % 16] = q[-1 - j]
        ids[b] = q[-1]
        if k == 3:                                                    # a near miss: one token of the sequence differs
            if len(q) == 1:
                ids[b] = 999
            else:
                tail[b, (g - 1 - int(rng.integers(0, len(q) - 1))) % 16] = 998
        if k == 5:
            sets[b] = 0
        if k == 1:
            sets[b] = -1 if b % 4 else 77                             # (77: outside the tables, no set either)
        pos[b] = -1 if k == 0 else start[b] + g
    return tables, ids, pos, sets, start, tail


@pytest.mark.parametrize("B", [1, 5, 8, 9, 64, 256])
def test_stop_step_entry_exact(hip, B):
    L = _lib.lib()
    tables, ids, pos, sets, start, tail = _step_case(B, B)
    host = SS.padded(tables, CAPS)
    w_pos, w_tail = pos.copy(), tail.copy()
    stop_step_np(ids, w_pos, host, sets, start, w_tail, MIN_NEW)
    quiet = (pos < 0) | (sets < 0) | (sets >= 4)
    assert np.array_equal(w_pos[quiet], pos[quiet]) and np.array_equal(w_tail[quiet], tail[quiet])
    assert w_pos[0] == -1 and (B < 64 or ((w_pos[~quiet] >= 0).sum() > B // 4 and (w_pos[~quiet] < 0).sum() > B // 8))
    T = [hip.from_numpy(a) for a in host]
    I, P, S, ST, TL = (hip.from_numpy(a) for a in (ids.reshape(B, 1), pos, sets, start, tail))
    MN = hip.from_numpy(np.array([MIN_NEW], np.int32))
    L.call("pdnh_stop_step", I._ptr, P._ptr, B, *(a._ptr for a in T), *CAPS, S._ptr, ST._ptr, TL._ptr, MN._ptr, hip.stream())
    assert np.array_equal(P.get(), w_pos) and np.array_equal(TL.get(), w_tail)
    assert np.array_equal(P.get()[quiet], pos[quiet]) and np.array_equal(TL.get()[quiet], tail[quiet])   # untouched rows
    for a, d in zip(host, T):                                         # the tables and the rest are only read
        assert np.array_equal(d.get(), a)
    assert np.array_equal(I.get().reshape(-1), ids) and np.array_equal(S.get(), sets) and np.array_equal(ST.get(), start)
    assert MN.get().tolist() == [MIN_NEW]
    # min_new = 0: the matches at g <= 2 count as well
    w_pos, w_tail = pos.copy(), tail.copy()
    stop_step_np(ids, w_pos, host, sets, start, w_tail, 0)
    P, TL, MN = hip.from_numpy(pos), hip.from_numpy(tail), hip.from_numpy(np.array([0], np.int32))
    L.call("pdnh_stop_step", I._ptr, P._ptr, B, *(a._ptr for a in T), *CAPS, S._ptr, ST._ptr, TL._ptr, MN._ptr, hip.stream())
    assert np.array_equal(P.get(), w_pos) and np.array_equal(TL.get(), w_tail)


@pytest.mark.parametrize("B", [3, 700])
def test_stop_reset_entry(hip, B):
    L = _lib.lib()
    rng = np.random.default_rng(B)
    state = [rng.integers(-1, 9, B).astype(np.int32), rng.integers(0, 50, B).astype(np.int32),
             rng.integers(0, 2500, (B, 16)).astype(np.int32)]
    R = 5 if B == 3 else 300                                          # (300 rows: more than one workgroup)
    rows = rng.permutation(B)[:R].astype(np.int32) if B > 3 else np.array([B - 1, 0, B + 5, 1, -1], np.int32)
    if B > 3:
        rows[7], rows[260] = B + 5, -1                                # outside: skipped
    src = (rng.integers(-1, 16, R).astype(np.int32), rng.integers(1, 2000, R).astype(np.int32),
           np.where(np.arange(R) % 2 == 0, -1, rng.integers(0, 2500, R)).astype(np.int32))
    want = [a.copy() for a in state]
    stop_reset_np(want, rows, src)
    listed = np.isin(np.arange(B), rows)
    assert all(np.array_equal(w[~listed], a[~listed]) for w, a in zip(want, state)) and (B == 3 or (~listed).sum() > 300)
    assert (want[2][listed][:, [0] + list(range(2, 16))] == -1).all() and (want[2][listed][:, 1] >= 0).any()
    # (the arrays sit inside a larger allocation: a write past row B - 1 or before row 0 would show)
    G = 64
    D = [hip.from_numpy(np.concatenate([np.full((G,) + a.shape[1:], 12345, np.int32), a,
                                        np.full((G,) + a.shape[1:], 12345, np.int32)])) for a in state]
    S, RW = [hip.from_numpy(a) for a in src], hip.from_numpy(rows)
    L.call("pdnh_stop_reset", D[0]._ptr + G * 4, D[1]._ptr + G * 4, D[2]._ptr + G * 16 * 4, B, RW._ptr, R, S[0]._ptr,
           S[1]._ptr, S[2]._ptr, hip.stream())
    for d, w in zip(D, want):
        got = d.get()
        assert np.array_equal(got[G:G + B], w) and (got[:G] == 12345).all() and (got[G + B:] == 12345).all()
    for d, a in zip(S + [RW], src + (rows,)):
        assert np.array_equal(d.get(), a)


def test_replayed_step_hands_the_tail_on(hip):
    """Three replays of one captured launch of the step kernel; the host plays the tick between them (a new token, the
    position one further).  The length-3 sequence completes on the third replay: pos is -1 afterwards and not before, and
    after every replay the tails are the host matcher's."""
    L = _lib.lib()
    B = 9
    a, b, c = 11, 12, 13
    spec = SS.check_args([[[a, b, c]], [[a, b, c], [b]], None, [[c, a]]] * 3, VOCAB, 12)
    host = SS.padded(spec.tables, spec.caps)
    T = [hip.from_numpy(x) for x in host]
    req = np.arange(B) % 4                                           # rows 1, 5: [b] ends them on the second replay
    lens = (3 + np.arange(B)).astype(np.int32)
    sets = spec.sets_of(req)
    pos0 = np.where(np.arange(B) == 4, -1, lens + 1).astype(np.int32)     # row 4 never runs
    S, ST = hip.from_numpy(np.zeros(B, np.int32)), hip.from_numpy(np.zeros(B, np.int32))
    TL = hip.from_numpy(np.zeros((B, 16), np.int32))
    I, P, MN = hip.from_numpy(np.full((B, 1), a, np.int64)), hip.from_numpy(pos0), hip.from_numpy(np.zeros(1, np.int32))
    RW, RS, RL, RF = (hip.from_numpy(x) for x in (np.arange(B, dtype=np.int32), sets, lens, np.full(B, -1, np.int32)))
    L.call("pdnh_stop_reset", S._ptr, ST._ptr, TL._ptr, B, RW._ptr, B, RS._ptr, RL._ptr, RF._ptr, hip.stream())
    rows = SS.Rows(B, spec)
    rows.reset(np.arange(B), req)
    assert np.array_equal(TL.get(), rows.tail) and (rows.tail == -1).all()

    def launches():
        L.call("pdnh_stop_step", I._ptr, P._ptr, B, *(x._ptr for x in T), *spec.caps, S._ptr, ST._ptr, TL._ptr, MN._ptr,
               hip.stream())
    keep = TL.copy()
    g = hip.Graph()
    g.capture(launches)                                              # (two real runs: the tails are put back, as _issue does)
    TL[...] = keep
    pos = pos0.copy()
    try:
        for it, tok in enumerate((a, b, c)):
            I[...] = np.full((B, 1), tok, np.int64)
            P[...] = pos
            g.replay()
            stopped = rows.feed(np.where(pos >= 0, tok, -1))
            got = P.get()
            assert np.array_equal(TL.get(), rows.tail), it
            assert np.array_equal(got < 0, stopped | (pos < 0)), it
            assert stopped.tolist() == [[False] * B, [r in (1, 5) for r in range(B)],
                                        [r in (0, 8) for r in range(B)]][it]
            pos = np.where(got >= 0, got + 1, -1).astype(np.int32)
    finally:
        g.destroy()
    assert rows.tail[0, 1:4].tolist() == [a, b, c] and rows.tail[3, 1:4].tolist() == [a, b, c] and pos[3] >= 0


# -- end to end ----------------------------------------------------------------------------------------------------
N_NEW = 40


def _ragged(m, prompts, n, **kw):
    return _run(m, lambda: _steps(m.generate_ragged(prompts, n, **kw)))


def _serve_all(m, prompts, budgets, **kw):
    return [o.tolist() for o in _run(m, lambda: m.serve_all(prompts, budgets, **kw))]


def _seqs_of(base):
    """Each request's stop sequences from its own output: tokens [5, 7) and [11, 14) of it; one request in four None."""
    return [None if r % 4 == 2 else [list(map(int, t[5:7])), list(map(int, t[11:14]))] for r, t in enumerate(base)]


def _cut(base, seqs):
    out = []
    for t, s in zip(base, seqs):
        g = SS.truncate(t, s)
        out.append(list(map(int, t if g is None else t[:g])))
    return out


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [1, 8, 16])
def test_generate_ragged_truncates(hip, B, kw):
    Graph.clear()
    prompts = _prompts(B, 40 + B)
    m0 = _model("hip:0", B)
    base = _ragged(m0, prompts, N_NEW, **kw)
    assert base.shape == (B, N_NEW) and m0._decode_st["graphs"] and m0._decode_st["stopseq"] is False
    seqs = _seqs_of(base)
    want = _cut(base, seqs)
    m = _model("hip:0", B)
    got = _ragged(m, prompts, N_NEW, stop_sequences=seqs[0] if B == 1 else seqs, **kw)
    st = m._decode_st
    assert st["stopseq"] and st["ok"] and st["graphs"] and st["wide"] == (B > 8)
    for r in range(B):
        k = len(want[r])
        assert got[r, :k].tolist() == want[r] and (got[r, k:] == -1).all(), r      # -1 from the next step on
    assert got.shape[1] == min(N_NEW, max(len(w) for w in want)) and (B > 1 or got.shape[1] <= 14)
    assert all(len(w) <= 14 for r, w in enumerate(want) if r % 4 != 2) and (B < 4 or len(want[2]) == N_NEW)
    # the capture's two real runs advanced the tails and were put back: the device's tails are the host matcher's
    rows = SS.Rows(B, SS.check_args(seqs[0] if B == 1 else seqs, VOCAB, B), np.arange(B))
    for s in range(got.shape[1]):
        rows.feed(got[:, s])
    assert np.array_equal(st["ss_tail"].get(), rows.tail) and st["ss_set"].get().tolist() == rows.set.tolist()
    assert st["ss_start"].get().tolist() == [p.size for p in prompts]
    stopped = np.array([len(w) < got.shape[1] for w in want])
    assert (st["pos"].get()[stopped] == -1).all()


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("chunk", [None, 16])
def test_serve_truncates(hip, chunk, kw):
    Graph.clear()
    N, slots = 14, 8
    prompts = _prompts(N, 60 + (chunk or 0))
    base = _serve_all(_model("hip:0", N), prompts, N_NEW, slots=slots, prefill_chunk=chunk, **kw)
    assert all(len(t) == N_NEW for t in base)
    seqs = _seqs_of(base)
    want = _cut(base, seqs)
    m = _model("hip:0", N)
    _counters()
    got = _serve_all(m, prompts, N_NEW, slots=slots, prefill_chunk=chunk, stop_sequences=seqs, **kw)
    c = _counters()
    st = m._decode_st
    assert got == want and st["stopseq"] and st["ok"] and st["graphs"] and c[53] > 0
    assert sum(len(w) <= 14 for w in want) == 11 and len(want[2]) == N_NEW
    assert (chunk is None) or any(len(k) > 2 and k[2] == "mixed" for k in st["graphs"])


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("chunk", [None, 16])
def test_served_device_state_follows_the_host(hip, monkeypatch, chunk, kw):
    """`serve` with nothing queued ahead: after every step the device's tails are the host matcher's, a row whose token
    ends a sequence is at -1 by the step kernel's store and a row that goes on is at start + g, on the served and on the
    mixed step (tests/test_stop_sequences.py: served_state_follows)."""
    Graph.clear()
    monkeypatch.setattr(Llama, "decode_ahead", False)
    N, slots = 14, 8
    prompts = _prompts(N, 80 + (chunk or 0))
    base = _serve_all(_model("hip:0", N), prompts, N_NEW, slots=slots, prefill_chunk=chunk, **kw)
    seqs = _seqs_of(base)
    m = _model("hip:0", N)
    seen = _run(m, lambda: served_state_follows(m, prompts, N_NEW, slots, chunk, seqs, _cut(base, seqs), **kw))
    st = m._decode_st
    assert seen >= 3 and st["stopseq"] and st["ok"] and st["graphs"]
    assert (chunk is None) or any(len(k) > 2 and k[2] == "mixed" for k in st["graphs"])


def test_plan_and_counters(hip, monkeypatch):
    """A graph-replayed run holds graphs and the stop state, and its replays do not pass through the entry; launch by launch
    the same tokens with one launch of the step kernel per step (plus the reset).  With stop_sequences at its default the
    plan key and every counter are those of a run without the keyword; with sequences only the new slot differs."""
    Graph.clear()
    n, B = 12, 4
    prompts = _prompts(B, 44)
    m = _model("hip:0", B)
    base = _ragged(m, prompts, n)
    never = [[int(np.setdiff1d(np.arange(VOCAB), base)[0]), 3]]      # (no row stops: the runs are like for like)
    m = _model("hip:0", B)
    _counters()
    got = _ragged(m, prompts, n, stop_sequences=never)
    c = _counters()
    st = m._decode_st
    assert np.array_equal(got, base) and st["stopseq"] and st["graphs"] and st["key"][-4:] == ("stopseq",) + CAPS
    assert 0 < c[53] < n and not st["full"]
    assert np.array_equal(st["ss_set_off"].get(), SS.padded(SS.check_args(never, VOCAB, B).tables, CAPS)[0])
    monkeypatch.setattr(Llama, "graph_decode", False)
    m = _model("hip:0", B)
    _counters()
    again = _ragged(m, prompts, n, stop_sequences=never)
    c_on = _counters()
    m = _model("hip:0", B)
    plain = _ragged(m, prompts, n)
    c_off = _counters()
    monkeypatch.setattr(Llama, "graph_decode", True)
    assert np.array_equal(again, base) and np.array_equal(plain, base) and not m._decode_st["graphs"]
    assert c_on[53] == (n - 1) + 1 and c_off[53] == 0                # one per step when on (and the reset), zero when off
    assert c_on[:53] == c_off[:53]                                   # every other counter: equal
    Graph.clear()
    m0, m1 = _model("hip:0", B), _model("hip:0", B)
    _counters()
    base = _ragged(m0, prompts, 10, stop_ids=[7])
    c0 = _counters()
    Graph.clear()
    again = _ragged(m1, prompts, 10, stop_ids=[7], stop_sequences=None)
    c1 = _counters()
    k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
    assert np.array_equal(base, again) and c0 == c1 and c0[53] == 0
    assert len(k0) == len(k1) == 11 and k0[:5] == k1[:5] and k0[6:] == k1[6:]      # (index 5: the weights' addresses)
    assert m1._decode_st["stopseq"] is False and "ss_tail" not in m1._decode_st and not m1._decode_st["full"]
