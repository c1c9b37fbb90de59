"""stop_sequences (llm/stop_sequences.py) without a GPU: the argument check, the oracle `truncate` and the host matcher
`Rows` on hand-made streams, and `generate_ragged` / `serve` / `serve_all` end to end on the emulated ABI
(tests/abi_emulator/_stopseq.py) with the small model of tests/test_logit_edits_gpu.py: a request's output with stop
sequences is its output without them, truncated at the match."""
import numpy as np
import pytest

from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import logit_edits as E
from pydynet_amd.llm import stop_sequences as SS
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, remove
from tests.abi_emulator import _stopseq
from tests.test_logit_edits_gpu import SAMPLED, VOCAB, _model, _prompts, _run, _steps

NSLOT = 54
V = VOCAB


# -- the argument ----------------------------------------------------------------------------------------------------
def test_check_args_forms():
    assert SS.check_args(None, V, 3) is None and SS.check_args([], V, 3) is None and SS.check_args((), V, 3) is None
    assert SS.check_args([None, None, []], V, 3) is None
    s = SS.check_args([[13, 13], (7,), [13, 13]], V, 3)               # shared; duplicates collapse
    assert s.sets == [((7,), (13, 13))] and s.set_of.tolist() == [0, 0, 0] and s.m == 0
    assert s.seqs(2) == ((7,), (13, 13))
    s = SS.check_args(np.array([[1, 2], [3, 4]]), V, 5, m=2)
    assert s.sets == [((1, 2), (3, 4))] and s.set_of.tolist() == [0] * 5 and s.m == 2
    p = SS.check_args([[[1, 2]], None, [[3], [1, 2]], [[1, 2]]], V, 4)  # per request; equal sets are held once
    assert p.sets == [((1, 2),), ((1, 2), (3,))] and p.set_of.tolist() == [0, -1, 1, 0] and p.seqs(1) == ()
    assert p.sets_of([2, -1, 1]).tolist() == [1, -1, -1]
    set_off, seq_off, toks = p.tables
    assert set_off.tolist() == [0, 1, 3] and seq_off.tolist() == [0, 2, 4, 5] and toks.tolist() == [1, 2, 1, 2, 3]
    assert all(a.dtype == np.int32 for a in p.tables) and p.caps == (16, 64, 256)
    a, b, c = SS.padded(p.tables, p.caps)
    assert a.shape == (17,) and b.shape == (65,) and c.shape == (256,) and a[2:].tolist() == [3] * 15 and b[3:].max() == 5
    with pytest.raises(ValueError):
        SS.padded(p.tables, (1, 64, 256))
    # three requests with three sequences each, all shared: depth tells the forms apart, not the count
    assert SS.check_args([[1], [2], [3]], V, 3).set_of.tolist() == [0, 0, 0]
    assert SS.check_args([[[1]], [[2]], [[3]]], V, 3).set_of.tolist() == [0, 1, 2]
    assert SS.packed([[(1, 2)], []], [1, -1, 0])[3].tolist() == [1, -1, 0]


BAD = [
    ([[1, 2], None], 2),                                              # a mixture of the two forms
    ([[1, 2], [[3]]], 2),
    ([[[1]], [[2]]], 3),                                              # per request: a wrong count
    ([[]], 1), ([[[]]], 1),                                           # an empty sequence
    ([list(range(17))], 1),                                           # MAX_LEN + 1 tokens
    ([[-1]], 1), ([[V]], 1), ([[1.5]], 1), ([[True]], 1), ([["a"]], 1),
    ([[[t] for t in range(17)]], 1),                                  # MAX_SEQS + 1 distinct sequences of one request
    (5, 1), ("ab", 1), ([1, 2], 1), (np.array([1, 2]), 1),
]


@pytest.mark.parametrize("bad,n", BAD)
def test_bad_arguments_raise(bad, n):
    with pytest.raises(ValueError):
        SS.check_args(bad, V, n)


def test_limits_and_other_arguments(emulated_hip):
    assert SS.check_args([[t] for t in range(16)] + [[3]], V, 1).set_of.tolist() == [0]      # 16 distinct: fine
    assert SS.check_args([list(range(16))], V, 1) is not None
    per = [[[r, t] for t in range(16)] for r in range(257)]                                  # 4112 sequences in all
    with pytest.raises(ValueError):
        SS.check_args(per, V, 257)
    assert SS.check_args(per[:256], V, 256).caps == (256, 4096, 8192)
    assert SS.check_args([[[1, t] for t in range(16)]] * 300, V, 300).caps == (16, 64, 256)  # equal sets: held once
    with pytest.raises(ValueError):
        SS.check_args([[1]], V, 1, speculate=2)
    with pytest.raises(ValueError):
        SS.check_args([[1]], V, 1, m=-1)
    # min_new_tokens: stop ids or stop sequences; with neither it raises as before
    with pytest.raises(ValueError):
        E.check_args(None, None, 3, V, 2)
    assert E.check_args(None, None, 3, V, 2, stop_sequences=True) is None
    assert E.check_args(None, None, 3, V, 2, [5], stop_sequences=True).m == 3
    m = _model("hip:0", 2)
    prompts = _prompts(2, 1)
    for kw in (dict(stop_sequences=[[1]], speculate=2), dict(stop_sequences=[[V]]), dict(min_new_tokens=2),
               dict(stop_sequences=[[1], None])):
        with pytest.raises(ValueError):
            m.generate_ragged(prompts, 4, **kw)
    for kw in (dict(stop_sequences=[[[1]]]), dict(stop_sequences=[[1, -1]]), dict(min_new_tokens=2)):
        with pytest.raises(ValueError):
            m.serve(prompts, 4, **kw)
        with pytest.raises(ValueError):
            m.serve_all(prompts, 4, **kw)
    with pytest.raises(TypeError):
        m.generate(np.stack([p[:1] for p in prompts]), 4, stop_sequences=[[1]])
    with pytest.raises(TypeError):
        m.beam_search(prompts, 4, 2, stop_sequences=[[1]])
    assert not any(c.startswith(("pdnh_", "pdn_decode")) for c in _lib._LIB.calls)           # nothing ran


# -- the oracle and the host matcher on hand-made streams ------------------------------------------------------------
def _feed_all(seqs, stream, m=0, first=False):
    """`Rows` with one row fed `stream` token by token (`first`: the first token through `reset`): the g at which it stops."""
    spec = SS.check_args([seqs], V, 1, m=m)
    rows = SS.Rows(1, spec)
    hits = []
    if first:
        hits.append(bool(rows.reset([0], [0], [stream[0]])[0]))
    else:
        rows.reset([0], [0])
    for t in stream[len(hits):]:
        hits.append(bool(rows.feed(np.array([t]))[0]))
    assert rows.count[0] == len(stream) and rows.first[0] == stream[0]
    return hits.index(True) + 1 if True in hits else None


A, B_, C = 5, 9, 11
LONG = list(range(100, 116))
STREAMS = [
    ([[A]], [B_, C, A, A], 0, 3),                                     # length 1
    ([LONG], [1, 2] + LONG + [3], 0, 18),                             # length 16, ending at g = 18: the ring has wrapped
    ([LONG], LONG[1:] + LONG, 0, 31),
    ([LONG], LONG[:15] + [7] + LONG[:15], 0, None),
    ([[A, B_, C], [B_, C]], [1, A, B_, C, 2], 0, 4),                  # one a suffix of the other
    ([[A, B_, C], [B_]], [1, A, B_, C, 2], 0, 3),                     # ... the shorter one ends first
    ([[A, A, B_]], [A, A, A, B_], 0, 4),                              # self-overlapping
    ([[A, B_]], [A, B_, 1], 0, 2),                                    # the seeded first token takes part
    ([[A]], [A, 1], 0, 1),
    ([[A, B_]], [B_, 1, 2], 0, None),                                 # prompt ... A | B_ ...: the prompt never takes part
    ([[C, A]], list(range(200, 220)) + [C, A], 0, 22),                # after more than 16 tokens
    ([[A, B_]], [A, B_, 1, A, B_, 2], 2, 5),                          # m = 2: the match ending at g = 2 is ignored
    ([[A, B_]], [A, B_, 1, A, B_, 2], 1, 2),                          # m = 1: g = 2 > m counts
    ([[A]], [A, A, A, 1], 2, 3),                                      # a length-1 sequence: the step of a stop id, g > m
    ([[A, B_]], [A, B_, 1], 5, None),
]


@pytest.mark.parametrize("seqs,stream,m,want", STREAMS)
def test_truncate_and_rows(seqs, stream, m, want):
    assert SS.truncate(stream, seqs, m) == want
    assert _feed_all(seqs, stream, m) == want
    assert _feed_all(seqs, stream, m, first=True) == want
    assert SS.truncate(stream, None) is None and SS.truncate(stream, []) is None


def test_rows_batch_and_reset():
    """Rows of a batch are independent, a row fed -1 is left as it is, and a row that takes a new request starts from a
    cleared tail: request 0 ends in A, request 1 starts with B_ -- no match across the two."""
    spec = SS.check_args([[[A, B_]], [[A, B_]], None], V, 3)
    rows = SS.Rows(3, spec, np.arange(3))
    assert rows.set.tolist() == [0, 0, -1]
    assert rows.feed(np.array([A, 1, A])).tolist() == [False] * 3
    assert rows.feed(np.array([-1, A, B_])).tolist() == [False] * 3 and rows.count.tolist() == [1, 2, 0]
    rows.reset([0], [1])                                              # row 0: request 1, whose first token is B_
    assert rows.tail[0].tolist() == [-1] * 16 and rows.count[0] == 0
    assert rows.feed(np.array([B_, B_, B_])).tolist() == [False, True, False]
    assert rows.reset([2, 0], [0, 1], [A, 7]).tolist() == [False, False] and rows.set.tolist() == [0, 0, 0]
    assert rows.feed(np.array([1, 1, B_])).tolist() == [False, False, True]


# -- end to end on the emulator --------------------------------------------------------------------------------------
N_NEW = 24


def _ragged(m, prompts, n, **kw):
    """(B, steps) tokens of generate_ragged, every step's rows."""
    return _run(m, lambda: _steps(m.generate_ragged(prompts, n, **kw)))


def _serve_all(m, prompts, budgets, **kw):
    return [o.tolist() for o in _run(m, lambda: m.serve_all(prompts, budgets, **kw))]


def _seqs_of(base):
    """Each request's stop sequences from its own output: tokens [5, 7) and [11, 14) of it; one request in four None."""
    return [None if r % 4 == 2 else [list(map(int, t[5:7])), list(map(int, t[11:14]))] for r, t in enumerate(base)]


def _cut(base, seqs, m=0):
    out = []
    for t, s in zip(base, seqs):
        g = SS.truncate(t, s, m)
        out.append(list(map(int, t if g is None else t[:g])))
    return out


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [1, 8])
def test_generate_ragged_truncates(emulated_hip, B, kw):
    _stopseq.extend()
    prompts = _prompts(B, 40 + B)
    base = _ragged(_model("hip:0", B), prompts, N_NEW, **kw)
    seqs = _seqs_of(base)
    if B == 1:
        seqs = seqs[0]                                                # (the shared form)
    want = _cut(base, seqs if B > 1 else [seqs])
    counters(NSLOT)
    m = _model("hip:0", B)
    got = _ragged(m, prompts, N_NEW, stop_sequences=seqs, **kw)
    c = counters(NSLOT)
    st = m._decode_st
    # one reset and one launch per decode step (and the step queued ahead when the run ended early)
    assert st["stopseq"] and st["ok"] and got.shape[1] <= c[53] <= got.shape[1] + 1
    for r in range(B):
        k = len(want[r])
        assert got[r, :k].tolist() == want[r] and (got[r, k:] == -1).all(), r      # -1 from the next step on
    # the iterator ends when every row has stopped
    assert got.shape[1] == min(N_NEW, max(len(w) for w in want)) and (B == 8 or got.shape[1] < N_NEW)
    assert any(len(w) < N_NEW for w in want) and (B < 4 or len(want[2]) == N_NEW)
    # the device's tails are the host matcher's, and a stopped row's position is -1 where it ran to the end
    rows = SS.Rows(B, SS.check_args(seqs, V, B), np.arange(B))
    for s in range(got.shape[1]):
        rows.feed(got[:, s])
    assert np.array_equal(st["ss_tail"].get(), rows.tail) and st["ss_set"].get().tolist() == rows.set.tolist()
    assert st["ss_start"].get().tolist() == [p.size for p in prompts]


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("slots,chunk", [(2, None), (8, None), (2, 4), (8, 4), (8, 64)])
def test_serve_truncates(emulated_hip, slots, chunk, kw):
    _stopseq.extend()
    N = 10
    prompts = _prompts(N, 60 + slots)
    base = _serve_all(_model("hip:0", N), prompts, N_NEW, slots=slots, prefill_chunk=chunk, **kw)
    assert all(len(t) == N_NEW for t in base)
    seqs = _seqs_of(base)
    want = _cut(base, seqs)
    counters(NSLOT)
    m = _model("hip:0", N)
    got = _serve_all(m, prompts, N_NEW, slots=slots, prefill_chunk=chunk, stop_sequences=seqs, **kw)
    assert got == want and counters(NSLOT)[53] > 0 and m._decode_st["stopseq"] and m._decode_st["ok"]
    assert sum(len(w) < N_NEW for w in want) >= 6 and len(want[2]) == N_NEW
    # stop ids and the budget act as before, whichever comes first
    budgets = [6 + (5 * r) % 17 for r in range(N)]
    stop = int(base[1][9])
    ref = []
    for t, s, b in zip(base, seqs, budgets):
        ends = [b, SS.truncate(t, s) or b] + ([t.index(stop) + 1] if stop in t else [])
        ref.append(t[:min(ends)])
    got = _serve_all(m, prompts, budgets, slots=slots, prefill_chunk=chunk, stop_sequences=seqs, stop_ids=[stop], **kw)
    assert got == ref


def served_state_follows(m, prompts, budget, slots, chunk, seqs, want, **kw):
    """`serve` step by step with nothing queued ahead, so that after a step the device holds exactly that step's state:
    every row that holds a request with sequences has the host matcher's tail; a row whose token ends a sequence is at
    position -1 -- stored by the step kernel, nothing else writes `pos` behind the tick -- and a row that goes on is at
    start + g, the position the kernel derives g from, in the plain and in the mixed step.  `want`: every request's
    expected tokens.  Returns how many stops were seen in steps where the host wrote no row state afterwards."""
    S, N = slots, len(prompts)
    rows = SS.Rows(S, SS.check_args(seqs, V, N))
    held, n_out, seen = np.full(S, -1, np.int64), [0] * N, 0
    for reqs, toks in m.serve(prompts, budget, slots=slots, prefill_chunk=chunk, stop_sequences=seqs, **kw):
        st = m._decode_st
        new = np.flatnonzero((reqs >= 0) & (reqs != held))
        rows.reset(new, reqs[new])
        held[new] = reqs[new]
        stopped = rows.feed(toks)
        pos, tail = st["pos"].get(), st["ss_tail"].get()
        for b in np.flatnonzero(held >= 0).tolist():
            r = int(held[b])
            n_out[r] += int(toks[b] >= 0)
            done = n_out[r] == len(want[r])
            if rows.set[b] >= 0:
                assert tail[b].tolist() == rows.tail[b].tolist(), (r, n_out[r])
            assert bool(stopped[b]) == (done and SS.truncate(want[r], rows.spec.seqs(r)) == n_out[r]), (r, n_out[r])
            if done:
                assert pos[b] == -1, (r, n_out[r], int(pos[b]))
                seen += int(stopped[b] and (chunk is not None or not new.size))
                held[b] = -1
            elif n_out[r]:
                assert pos[b] == prompts[r].size + n_out[r], (r, n_out[r], int(pos[b]))
    assert n_out == [len(w) for w in want]
    return seen


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("slots,chunk", [(3, None), (10, None), (3, 4), (10, 64)])
def test_served_device_state_follows_the_host(emulated_hip, monkeypatch, slots, chunk, kw):
    _stopseq.extend()
    monkeypatch.setattr(Llama, "decode_ahead", False)
    N = 10
    prompts = _prompts(N, 70 + slots)
    base = _serve_all(_model("hip:0", N), prompts, N_NEW, slots=slots, prefill_chunk=chunk, **kw)
    seqs = _seqs_of(base)
    m = _model("hip:0", N)
    seen = _run(m, lambda: served_state_follows(m, prompts, N_NEW, slots, chunk, seqs, _cut(base, seqs), **kw))
    assert seen >= 3 and m._decode_st["stopseq"] and m._decode_st["ok"]


def test_run_resumed_on_the_plan_keeps_its_ring(emulated_hip):
    """A generation that comes back after another one replaced its plan takes its whole ring along, not only its first
    token: a sequence that spans the interruption still stops the row on the device.  (The other generation runs in cache
    row 0, whose request is lost to it; rows 1 .. 3 keep their caches and go on.)"""
    _stopseq.extend()
    B = 4
    prompts = _prompts(B, 23)
    m = _model("hip:0", B)
    base = _ragged(m, prompts, 12)
    seqs = [[list(map(int, t[4:8]))] for t in base]
    it = m.generate_ragged(prompts, 12, stop_sequences=seqs)

    def both():
        out = [next(it).numpy().reshape(-1) for _ in range(6)]          # y_1 .. y_6: the first half of every match
        key = m._decode_st["key"]
        assert _steps(m.generate_ragged(prompts[:1], 3)).shape == (1, 3) and m._decode_st["key"] != key
        return np.stack(out + [t.numpy().reshape(-1) for t in it], 1)
    got = _run(m, both)
    st = m._decode_st
    assert st["stopseq"] and st["B"] == B
    assert np.array_equal(got[1:, :8], base[1:, :8]) and (got[1:, 8:] == -1).all() and (st["pos"].get()[1:] == -1).all()
    rows = SS.Rows(B, SS.check_args(seqs, V, B), np.arange(B))
    for s in range(got.shape[1]):
        rows.feed(got[:, s])
    assert np.array_equal(st["ss_tail"].get()[1:], rows.tail[1:])


def test_serve_steps_free_the_slot(emulated_hip):
    """In `serve` the row yields its matching token, and the next admission takes the freed slot at the next step."""
    _stopseq.extend()
    prompts = _prompts(3, 5)
    base = _serve_all(_model("hip:0", 3), prompts, 12, slots=1)
    seqs = [list(map(int, base[0][3:5]))]
    g = SS.truncate(base[0], seqs)
    m = _model("hip:0", 3)
    steps = _run(m, lambda: [(r.tolist(), t.tolist()) for r, t in m.serve(prompts, 12, slots=1, stop_sequences=[seqs, None, None])])
    assert [t[0] for r, t in steps if r[0] == 0] == base[0][:g]
    assert steps[g - 1][0] == [0] and steps[g][0] == [1] and steps[g][1] == [base[1][0]]


@pytest.mark.parametrize("kw", [{}, SAMPLED])
def test_single_token_sequence_equals_stop_id(emulated_hip, kw):
    """stop_sequences=[[t]] gives the same tokens, step by step, as stop_ids=[t] -- with min_new_tokens too, where the stop
    id is masked (so its runs differ from the plain ones) and the sequence is only ignored: compared where both apply."""
    _stopseq.extend()
    B = 8
    prompts = _prompts(B, 21)
    base = _ragged(_model("hip:0", B), prompts, 16, **kw)
    t = int(base[3][4])
    a = _ragged(_model("hip:0", B), prompts, 16, stop_ids=[t], **kw)
    b = _ragged(_model("hip:0", B), prompts, 16, stop_sequences=[[t]], **kw)
    assert np.array_equal(a, b) and (a[3, 5:] == -1).all()
    ma, mb = _model("hip:0", B), _model("hip:0", B)
    sa = _run(ma, lambda: [(r.tolist(), k.tolist()) for r, k in ma.serve(prompts, 16, slots=3, stop_ids=[t], **kw)])
    sb = _run(mb, lambda: [(r.tolist(), k.tolist()) for r, k in mb.serve(prompts, 16, slots=3, stop_sequences=[[t]], **kw)])
    assert sa == sb
    # min_new_tokens = m: a stop id may be yielded from g = m + 1 on; so may the sequence's match count
    m = 6
    got = _ragged(_model("hip:0", B), prompts, 16, stop_sequences=[[t]], min_new_tokens=m, **kw)
    for r in range(B):
        g = SS.truncate(base[r], [[t]], m)
        assert g is None or g > m
        k = 16 if g is None else g
        assert got[r, :k].tolist() == base[r, :k].tolist() and (got[r, k:] == -1).all()
    assert SS.truncate(base[3], [[t]], m) != 5 and got[3, 5] == base[3, 5]
    # ... and with a stop id as well the edit masks the id while the sequence is held back to the same step
    both = _ragged(_model("hip:0", B), prompts, 16, stop_ids=[t], stop_sequences=[[t]], min_new_tokens=m, **kw)
    only = _ragged(_model("hip:0", B), prompts, 16, stop_ids=[t], min_new_tokens=m, **kw)
    assert np.array_equal(both, only)


def test_new_request_does_not_match_on_the_old_tail(emulated_hip):
    """A served row that takes a new request starts from a cleared tail: request 0's last tokens followed by request 1's
    first would match, and must not."""
    _stopseq.extend()
    prompts = _prompts(2, 9)
    base = _serve_all(_model("hip:0", 2), prompts, 8, slots=1)
    for chunk in (None, 4):
        straddle = [int(base[0][3]), int(base[1][0])]                 # request 0 is cut to 4 tokens by its budget
        m = _model("hip:0", 2)
        got = _serve_all(m, prompts, [4, 8], slots=1, prefill_chunk=chunk, stop_sequences=[straddle])
        assert SS.truncate(base[0][:4] + base[1], [straddle]) == 5 and SS.truncate(base[1], [straddle]) is None
        assert got == [base[0][:4], base[1]] and m._decode_st["stopseq"]


def test_default_plan_and_counters_unchanged(emulated_hip):
    """With stop_sequences at its default (or empty) the plan key, the launches and the counters are those of a run without
    the keyword; with sequences the key grows by the term and the capacity, and a later call of similar size keeps the plan."""
    _stopseq.extend()
    runtime = ("pdn_malloc", "pdn_free", "pdn_set_device", "pdn_compute_stream", "pdn_fill", "pdn_kernel_counters",
               "pdn_memcpy")                                   # (allocator / setup traffic differs between first uses)

    def run(fn):
        _lib._LIB.calls.clear()
        counters(NSLOT)
        out = fn()
        return out, counters(NSLOT), [c for c in _lib._LIB.calls if not c.startswith(runtime)]
    prompts = _prompts(3, 11)
    m0, m1 = _model("hip:0", 3), _model("hip:0", 3)
    base, c0, calls0 = run(lambda: _ragged(m0, prompts, 6, stop_ids=[5]))
    again, c1, calls1 = run(lambda: _ragged(m1, prompts, 6, stop_ids=[5], stop_sequences=None))
    k0 = m0._decode_st["key"]
    assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[53] == 0
    assert not any("pdnh_" in c for c in calls0) and m1._decode_st["key"][:5] == k0[:5] and len(m1._decode_st["key"]) == len(k0)
    assert m1._decode_st["stopseq"] is False and "ss_tail" not in m1._decode_st
    for off in ([], [None] * 3):
        again, c1, calls1 = run(lambda: _ragged(m1, prompts, 6, stop_ids=[5], stop_sequences=off))
        assert np.array_equal(base, again) and c0 == c1 and len(m1._decode_st["key"]) == len(k0)
    for chunk in (None, 2):
        base, c0, calls0 = run(lambda: _serve_all(m0, prompts, 5, slots=2, prefill_chunk=chunk))
        again, c1, calls1 = run(lambda: _serve_all(m1, prompts, 5, slots=2, prefill_chunk=chunk, stop_sequences=[]))
        assert base == again and c0 == c1 and calls0 == calls1 and c0[53] == 0
    _ragged(m1, prompts, 6, stop_sequences=[[1, 2]])
    key = m1._decode_st["key"]
    assert key[-4:] == ("stopseq", 16, 64, 256) and len(key) == len(k0) + 4
    _ragged(m1, prompts, 6, stop_sequences=[[[3]], None, [[4, 5], [6]]])
    assert m1._decode_st["key"] == key


@pytest.mark.parametrize("graphs", [True, False])
def test_generic_path_agrees(emulated_hip, monkeypatch, graphs):
    """Without pdnh_stop_step the plan refuses and every path stops its rows by the host matcher: the same tokens, none of
    the entries launched."""
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    B = 5
    prompts = _prompts(B, 33)
    base = _ragged(_model("hip:0", B), prompts, N_NEW)
    seqs = _seqs_of(base)
    served = _serve_all(_model("hip:0", B), prompts, N_NEW, slots=2)
    want_r = None
    for removed in (False, True):
        Graph.clear()
        emu = _stopseq.extend()
        if removed:
            remove(monkeypatch, emu, "pdnh_stop_step")
        assert _lib.provides("pdnh_stop_step") is not removed
        counters(NSLOT)
        m = _model("hip:0", B)
        got = _ragged(m, prompts, N_NEW, stop_sequences=seqs)
        c = counters(NSLOT)
        assert m._decode_st["ok"] is not removed and (c[53] == 0) is removed
        want_r = got if want_r is None else want_r
        assert np.array_equal(got, want_r)
        assert [r[r >= 0].tolist() for r in got] == _cut(base, seqs)
        for chunk in (None, 4):
            assert _serve_all(_model("hip:0", B), prompts, N_NEW, slots=2, prefill_chunk=chunk,
                              stop_sequences=seqs) == _cut(served, seqs)


def test_cpu_device_agrees():
    """The tape-node path (`cpu`): the same rule from the host matcher alone."""
    B = 4
    prompts = _prompts(B, 17)
    m = _model("cpu", B)
    base = _ragged(m, prompts, 16)
    seqs = _seqs_of(base)
    got = _ragged(_model("cpu", B), prompts, 16, stop_sequences=seqs)
    assert [r[r >= 0].tolist() for r in got] == _cut(base, seqs)
    for chunk in (None, 3):
        assert _serve_all(_model("cpu", B), prompts, 16, slots=2, prefill_chunk=chunk, stop_sequences=seqs) == _cut(
            _serve_all(_model("cpu", B), prompts, 16, slots=2, prefill_chunk=chunk), seqs)


def test_emulated_entries_follow_the_statement(emulated_hip):
    """The emulated reset / step entries through the library's call path against `Rows` on a random walk: a vocabulary of 3
    tokens, so matches are frequent."""
    emu = _stopseq.extend()
    rng = np.random.default_rng(3)
    B = 9
    spec = SS.check_args([[[0, 1]], None, [[2], [1, 1, 0]], [[0, 1, 2, 0]], [[1, 0]]] * 2, 3, 10, m=2)
    caps = spec.caps
    T = [np.ascontiguousarray(a) for a in SS.padded(spec.tables, caps)]
    sets, start, tail = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.zeros((B, 16), np.int32)
    rows = SS.Rows(B, spec)
    req = rng.integers(0, 10, B)
    lens = rng.integers(1, 9, B).astype(np.int32)
    first = rng.integers(0, 3, B).astype(np.int32)
    first[::3] = -1
    r32 = np.arange(B, dtype=np.int32)
    s_set = spec.sets_of(req)
    assert emu.pdnh_stop_reset(sets.ctypes.data, start.ctypes.data, tail.ctypes.data, B, r32.ctypes.data, B,
                               s_set.ctypes.data, lens.ctypes.data, first.ctypes.data, 0) == 0
    rows.reset(np.arange(B), req)
    live = ~rows.feed(first)
    pos = np.where(live, lens + (first >= 0), -1).astype(np.int32)
    mn = np.array([spec.m], np.int32)
    stops = 0
    for _ in range(40):
        ids = rng.integers(0, 3, B)
        pos = np.where(pos >= 0, pos + 1, -1).astype(np.int32)        # (the tick: the row moves behind its new token)
        want = rows.feed(np.where(pos >= 0, ids, -1))
        assert emu.pdnh_stop_step(ids.ctypes.data, pos.ctypes.data, B, *(a.ctypes.data for a in T), *caps,
                                  sets.ctypes.data, start.ctypes.data, tail.ctypes.data, mn.ctypes.data, 0) == 0
        assert np.array_equal(pos < 0, want | ~live) and np.array_equal(tail[sets >= 0], rows.tail[sets >= 0])
        live = pos >= 0
        stops += int(want.sum())
        back = np.flatnonzero(~live)[:2].astype(np.int32)             # stopped rows take new requests, first token later
        if back.size:
            req[back] = rng.integers(0, 10, back.size)
            none = np.full(back.size, -1, np.int32)
            s_set = spec.sets_of(req[back])
            assert emu.pdnh_stop_reset(sets.ctypes.data, start.ctypes.data, tail.ctypes.data, B, back.ctypes.data,
                                       int(back.size), s_set.ctypes.data, lens[back].ctypes.data, none.ctypes.data, 0) == 0
            rows.reset(back, req[back])
            pos[back] = lens[back]
            live = pos >= 0
    assert stops > 10 and counters(NSLOT)[53] > 40
