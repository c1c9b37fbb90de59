"""Penalties on a real MI355X: the entries of csrc/penalty.hip bit for bit against the float32 statement
(tests/abi_emulator/_penalty.py), the plan's counts after a graph-replayed run, and `generate`, `generate_ragged` and
`serve` (plain and chunked) end to end against the `cpu` device under the first-difference margin rule of
tests/test_serve_gpu.py, on the narrow (<= 8 rows) and the wide step."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import penalties
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import apply_np, margin, penalty_chunks as chunks, reset_np

pytestmark = pytest.mark.gpu
f32 = np.float32
PEN = dict(repetition_penalty=1.6, presence_penalty=0.8, frequency_penalty=0.3)
SAMPLED = dict(temperature=0.9, top_p=0.92, seed=31)


def _rows_case(B, V, seed):
    rng = np.random.default_rng(seed)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    z[:, ::97] = 0.0
    z[:, 5::131] = -0.0
    z[:, 7::101] = -np.inf
    z[:, 11::211] = np.inf
    counts = np.where(rng.random((B, V)) < 0.05, rng.integers(1, 4, (B, V)), 0).astype(np.int32)
    counts[:, 3::509] = 70000                                        # large counts
    prompts = [rng.integers(0, V, int(n)) for n in rng.integers(0, 40, B)]
    pos = rng.integers(0, 60, B).astype(np.int32)
    pos[::3] = -1                                                    # skipped rows stay untouched
    start = rng.integers(0, 60, B).astype(np.int32)
    ids = rng.integers(0, V, B).astype(np.int64)
    return z, counts, prompts, pos, start, ids


@pytest.mark.parametrize("V", [32000, 1001])
@pytest.mark.parametrize("B", [1, 8, 64, 256])
def test_apply_entries_bit_equal(hip, B, V):
    L = _lib.lib()
    z, counts, prompts, pos, start, ids = _rows_case(B, V, B + V)
    seen = penalties.seen_bits(prompts, V)
    vals = (1.7, 0.45, 0.3)
    n = L.query("pdn_penalty_chunks", V)
    assert n == chunks(V)
    prm = hip.from_numpy(penalties.params_bytes(*vals))
    # the step's form: count the fed token, penalise, candidates
    want, wc = z.copy(), counts.astype(np.int64)
    cv, ci = apply_np(want, vals, wc, seen, pos, start, ids, count=True)
    Z, C, S = hip.from_numpy(z), hip.from_numpy(counts), hip.from_numpy(seen)
    P, ST, I = hip.from_numpy(pos), hip.from_numpy(start), hip.from_numpy(ids)
    CV, CI = hip.from_numpy(np.full((B, n), 7.0, f32)), hip.from_numpy(np.full((B, n), -7, np.int32))
    L.call("pdn_penalty_step_f32", Z._ptr, V, B, V, prm._ptr, C._ptr, S._ptr, ST._ptr, I._ptr, P._ptr, 1, CV._ptr,
           CI._ptr, hip.stream())
    got = Z.get()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(C.get(), wc.astype(np.int32))
    live = pos >= 0
    assert np.array_equal(CV.get()[live].view(np.int32), cv[live].view(np.int32))
    assert np.array_equal(CI.get()[live], ci[live])
    assert (CV.get()[~live] == 7.0).all() and (CI.get()[~live] == -7).all()
    # the standalone form: no counting, no plan; counts / prompt bits optional
    want = z.copy()
    apply_np(want, vals, counts.astype(np.int64), seen, pos)
    Z, C = hip.from_numpy(z), hip.from_numpy(counts)
    L.call("pdn_penalty_rows_f32", Z._ptr, V, B, V, prm._ptr, C._ptr, S._ptr, P._ptr, None, None, hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32)) and np.array_equal(C.get(), counts)
    want = z.copy()
    apply_np(want, vals, None, seen, None)
    Z = hip.from_numpy(z)
    L.call("pdn_penalty_rows_f32", Z._ptr, V, B, V, prm._ptr, None, S._ptr, None, None, None, hip.stream())
    assert np.array_equal(Z.get().view(np.int32), want.view(np.int32))


def test_step_entry_row_stride_and_shared_position(hip):
    """A logits row stride wider than V, and the rectangular form (pos_per_row = 0: every row at pos[0])."""
    L = _lib.lib()
    B, V, rs = 5, 3001, 3072
    z, counts, prompts, _, start, ids = _rows_case(B, V, 5)
    seen = penalties.seen_bits(prompts, V)
    vals = (0.8, -0.5, 1.25)                                         # r < 1 and a negative presence: allowed
    zz = np.full((B, rs), 3.0, f32)
    zz[:, :V] = z
    want, wc = z.copy(), counts.astype(np.int64)
    apply_np(want, vals, wc, seen, np.full(B, 30), start, ids, count=True)
    Z, C, S = hip.from_numpy(zz), hip.from_numpy(counts), hip.from_numpy(seen)
    P, ST, I = hip.from_numpy(np.array([30], np.int32)), hip.from_numpy(start), hip.from_numpy(ids)
    prm = hip.from_numpy(penalties.params_bytes(*vals))
    L.call("pdn_penalty_step_f32", Z._ptr, rs, B, V, prm._ptr, C._ptr, S._ptr, ST._ptr, I._ptr, P._ptr, 0, None, None,
           hip.stream())
    got = Z.get()
    assert np.array_equal(got[:, :V].view(np.int32), want.view(np.int32)) and (got[:, V:] == 3.0).all()
    assert np.array_equal(C.get(), wc.astype(np.int32))


@pytest.mark.parametrize("B,V", [(3, 32000), (70, 1001)])
def test_reset_entry(hip, B, V):
    L = _lib.lib()
    rng = np.random.default_rng(B)
    counts = rng.integers(0, 9, (B, V)).astype(np.int32)
    seen = rng.integers(-2 ** 31, 2 ** 31 - 1, (B, -(-V // 32))).astype(np.int32)
    start = rng.integers(0, 50, B).astype(np.int32)
    rows = np.array([B - 1, 0, B + 5, 1], np.int32)                   # B + 5: outside, skipped
    prompts = [rng.integers(0, V, 33), np.zeros(0, np.int64), rng.integers(0, V, 4), np.array([V - 1, 0, V - 1])]
    ids, off = penalties.packed(prompts)
    wc, ws, wst = counts.copy(), seen.copy(), start.copy()
    reset_np(wc, ws, wst, rows, ids, off)
    C, S, ST = hip.from_numpy(counts), hip.from_numpy(seen), hip.from_numpy(start)
    R, ID, OF = hip.from_numpy(rows), hip.from_numpy(ids), hip.from_numpy(off)
    L.call("pdn_penalty_reset", C._ptr, S._ptr, ST._ptr, B, V, R._ptr, 4, ID._ptr, OF._ptr, hip.stream())
    assert np.array_equal(C.get(), wc) and np.array_equal(S.get(), ws) and np.array_equal(ST.get(), wst)


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


def _reference(prompts, n, stops=(), **kw):
    """generate_ragged on `cpu` with every step's PENALISED logits (the statement on the recorded projections)."""
    m = _model("cpu", len(prompts))
    raw = []
    fwd = m.lm_head.forward

    def rec(x):
        y = fwd(x)
        raw.append(np.asarray(y.numpy(), np.float32)[:, -1, :])
        return y
    m.lm_head.forward = rec
    try:
        toks = _run(m, lambda: np.stack([t.numpy().reshape(-1) for t in
                                         m.generate_ragged(prompts, n, stop_ids=stops, **kw, **PEN)], 1))
    finally:
        del m.lm_head.forward
    vals = penalties.check_args(**PEN)
    seen = penalties.seen_rows(prompts, VOCAB)
    logits = []
    for s, z in enumerate(raw):
        c = np.zeros((len(prompts), VOCAB), np.int64)
        for r in range(len(prompts)):
            prev = toks[r, :s]
            np.add.at(c[r], prev[prev >= 0], 1)
        logits.append(penalties.penalize(z, c, seen, *vals))
    return toks, logits


def _check(got, ref, logits, prompts, budgets, stops, kw):
    """The first token that differs from the reference must sit at a float64 margin below 1e-5; up to it, equal."""
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
        z = logits[s][r]
        if kw:
            mg = margin(z, len(prompts[r]) + s, r, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw["seed"])
        else:
            srt = np.sort(z.astype(np.float64))
            mg = srt[-1] - srt[-2]
        assert mg < 1e-5, (r, s, mg)


def _prompts(N, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, VOCAB, 1 + (7 * r) % 11) for r in range(N)]


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [1, 8, 16, 64])
def test_generate_ragged_and_generate(hip, B, kw):
    Graph.clear()
    prompts = _prompts(B, B)
    n = 14
    ref, logits = _reference(prompts, n, **kw)
    stops = {int(ref[0, 5])}
    m = _model("hip:0", B)
    got = _run(m, lambda: np.stack([t.numpy().reshape(-1) for t in m.generate_ragged(prompts, n, **kw, **PEN)], 1))
    _check(got, ref, logits, prompts, [n] * B, set(), kw)
    assert m._decode_st["pen"] and m._decode_st["wide"] == (B > 8)
    ref_s, logits_s = _reference(prompts, n, stops, **kw)
    m = _model("hip:0", B)                           # (a fresh cache: a step reads the slot after its prompt unwritten)
    got = _run(m, lambda: np.stack([t.numpy().reshape(-1) for t in
                                    m.generate_ragged(prompts, n, stop_ids=stops, **kw, **PEN)], 1))
    _check([r[r >= 0] for r in got], ref_s, logits_s, prompts, [n] * B, stops, kw)
    # generate: equal lengths, the rectangular step
    ids = np.stack([np.resize(p, 6) for p in prompts])
    ref, logits = _reference(list(ids), n, **kw)
    m = _model("hip:0", B)
    got = _run(m, lambda: np.stack([t.numpy().reshape(-1) for t in m.generate(ids, 6 + n, **kw, **PEN)], 1))
    _check(got, ref, logits, list(ids), [n] * B, set(), kw)


def test_counts_after_graph_replayed_run(hip):
    """The plan's counts are the bincount of the tokens fed to its steps: the capture's two runs left nothing."""
    Graph.clear()
    for B in (4, 12):
        prompts = _prompts(B, 40 + B)
        m = _model("hip:0", B)
        got = _run(m, lambda: np.stack([t.numpy().reshape(-1) for t in m.generate_ragged(prompts, 12, **PEN)], 1))
        want = np.zeros((B, VOCAB), np.int64)
        for b in range(B):
            np.add.at(want[b], got[b, :-1], 1)
        st = m._decode_st
        assert st["pen"] and st["graphs"] and np.array_equal(st["counts"].get(), want)


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("slots,chunk", [(8, None), (8, 6), (16, None), (16, 8), (64, None)])
def test_serve(hip, slots, chunk, kw):
    Graph.clear()
    N = slots + 6
    prompts = _prompts(N, slots + (chunk or 0))
    budgets = [2 + (5 * r) % 13 for r in range(N)]
    ref, logits = _reference(prompts, int(max(budgets)), **kw)
    m = _model("hip:0", N)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=slots, prefill_chunk=chunk, **kw, **PEN))
    _check(got, ref, logits, prompts, budgets, set(), kw)


def test_huge_presence_never_repeats_and_nothing_leaks(hip):
    Graph.clear()
    prompts = _prompts(7, 77)
    m = _model("hip:0", 7)
    got = _run(m, lambda: np.stack([t.numpy().reshape(-1) for t in
                                    m.generate_ragged(prompts, 24, presence_penalty=1e4)], 1))
    for r in got:
        assert len(set(r.tolist())) == r.size
    big = dict(presence_penalty=1e4, repetition_penalty=2.0)
    budgets = [20, 9, 15, 12, 18, 6, 11]
    for chunk in (None, 4):
        served = _run(m, lambda: m.serve_all(prompts, budgets, slots=2, prefill_chunk=chunk, **big))
        for r, toks in enumerate(served):
            assert len(set(toks.tolist())) == toks.size
            alone = _run(m, lambda: m.serve_all([prompts[r]], [budgets[r]], slots=2, prefill_chunk=chunk, **big))[0]
            assert np.array_equal(toks, alone), r
