"""Sampling parameters per row and min_p on a real MI355X (include/pdn_persample.h): the standalone entry and the ticks bit for
bit against the shared-parameter entries called on one row with that row's block, the min_p rows against the NumPy statement
under the margin rule of tests/abi_emulator/_persample.py, and generate_ragged / serve_all with one parameter set per request
against the uniform runs with that request's values."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling as S
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator._persample import draw_np, margin, read_block

pytestmark = pytest.mark.gpu
f32 = np.float32
# the five blocks: greedy, plain, top_k = 1, top_p = 0.5, min_p = 0.3
KINDS = [dict(temperature=0.0), dict(temperature=1.0), dict(temperature=1.0, top_k=1), dict(temperature=1.0, top_p=0.5),
         dict(temperature=1.0, min_p=0.3)]


def _counters():
    buf = (ctypes.c_int64 * 50)()
    _lib.lib().call("pdn_kernel_counters", buf, 50, 1)
    return [int(v) for v in buf]


def _table(kinds):
    kw = [dict(dict(temperature=0.0, top_k=0, top_p=1.0, min_p=0.0, seed=1000 + 37 * b), **KINDS[k]) for b, k in enumerate(kinds)]
    return S.Table(**{n: [k[n] for k in kw] for n in ("temperature", "top_k", "top_p", "seed", "min_p")})


def _case(V, kinds, seed):
    """Logit rows (a few units apart: peaked distributions), the rows' blocks, positions and counter ids."""
    rng = np.random.default_rng(seed)
    B = len(kinds)
    z = (4 * rng.standard_normal((B, V))).astype(f32)
    return z, _table(kinds), rng.integers(0, 200, B).astype(np.int32), rng.integers(0, 1000, B).astype(np.int32)


def _against_the_statement(z, blocks, pos, ids, got):
    """The margin rule: a token that differs from the NumPy statement's is excused only where the float64 margin of that
    draw is below 1e-5, at most once per test.  The fixed inputs were chosen so that the statement itself has no draw
    under the margin (held here too), so in effect every token must equal the statement's."""
    excused = 0
    for b in range(len(z)):
        if pos[b] < 0:
            continue
        T, k, p, seed, m = read_block(blocks[b])
        mg = margin(z[b], int(pos[b]), int(ids[b]), T, k, p, seed, m) if T > 0 else float(np.diff(np.sort(z[b])[-2:])[0])
        assert mg >= 1e-5, ("the fixed input has a draw under the margin", b, mg)
        want = draw_np(z[b], blocks[b], int(pos[b]), int(ids[b]))
        if int(got[b]) != want:
            assert mg < 1e-5, (b, int(got[b]), want, mg)
            excused += 1
    assert excused <= 1, excused


@pytest.mark.parametrize("V", [1000, 4100, 32000])
def test_standalone_entry_equals_the_shared_entry_row_by_row(hip, V):
    L = _lib.lib()
    B, rs = 5, V + 4                                   # (a row stride past V)
    z, tab, pos, req = _case(V, range(5), V)
    buf = np.zeros((B, rs), f32)
    buf[:, :V] = z
    blocks = tab.blocks(range(B))
    Z, PRM, P, R = hip.from_numpy(buf), hip.from_numpy(blocks), hip.from_numpy(pos), hip.from_numpy(req)
    zero = hip.from_numpy(np.zeros(B, np.int32))
    _counters()
    out = hip.from_numpy(np.full(B, -7, np.int64))
    L.call("pdnq_sample_rows_f32", Z._ptr, rs, B, V, PRM._ptr, P._ptr, zero._ptr, out._ptr, hip.stream())
    c = _counters()
    assert c[49] == 1 and c[28] == 1
    got0 = out.get()
    out = hip.from_numpy(np.full(B, -7, np.int64))
    L.call("pdnq_sample_rows_f32", Z._ptr, rs, B, V, PRM._ptr, P._ptr, R._ptr, out._ptr, hip.stream())
    got = out.get()
    out = hip.from_numpy(np.full(B, -7, np.int64))
    L.call("pdnq_sample_rows_f32", Z._ptr, rs, B, V, PRM._ptr, P._ptr, None, out._ptr, hip.stream())
    got_rows = out.get()
    for b in range(B):
        one = hip.from_numpy(blocks[b])
        # the shared standalone entry on row b alone: counter (pos[b], 0)
        o1 = hip.from_numpy(np.full(1, -7, np.int64))
        L.call("pdn_sample_rows_f32", Z._ptr + 4 * b * rs, rs, 1, V, one._ptr, int(pos[b]), o1._ptr, hip.stream())
        # the shared slot tick on row b alone: counter (pos[b], req[b]) / (pos[b], b)
        o2 = []
        for cid in (int(req[b]), b):
            ids = hip.from_numpy(np.full(1, -7, np.int64))
            st = [hip.from_numpy(np.array([v], np.int32)) for v in (pos[b], 0, cid, 5)]
            L.call("pdn_decode_sample_tick_slots_f32", Z._ptr + 4 * b * rs, rs, 1, V, one._ptr, ids._ptr, st[0]._ptr,
                   st[1]._ptr, st[2]._ptr, st[3]._ptr, 1, None, None, None, 0, 0, None, hip.stream())
            o2.append(int(ids.get()[0]))
        # the same device function on the same row, block and counter: bit for bit (the shared entries never read min_p,
        # so the fifth row is held to the statement alone, below)
        if tab.min_p[b] == 0:
            assert (int(got0[b]), int(got[b]), int(got_rows[b])) == (int(o1.get()[0]), o2[0], o2[1]), b
    assert got[0] == z[0].argmax() and got[2] == z[2].argmax()          # greedy, and top_k = 1
    _against_the_statement(z, blocks, pos, req, got)
    _against_the_statement(z, blocks, pos, np.arange(B), got_rows)
    _against_the_statement(z, blocks, pos, np.zeros(B, np.int64), got0)
    # a row at a position < 0 is left alone, whatever its block holds
    pos2 = pos.copy()
    pos2[3] = -1
    blocks2 = blocks.copy()
    blocks2[3] = np.array([-1, -1, -1], np.int64)                        # (NaN temperature, top_k -1 ...: never read)
    out = hip.from_numpy(np.full(B, -7, np.int64))
    PRM2, P2 = hip.from_numpy(blocks2), hip.from_numpy(pos2)          # (held until the call has run)
    L.call("pdnq_sample_rows_f32", Z._ptr, rs, B, V, PRM2._ptr, P2._ptr, R._ptr, out._ptr, hip.stream())
    assert out.get().tolist() == [int(t) if b != 3 else -7 for b, t in enumerate(got)]


@pytest.mark.parametrize("V", [1000, 4100, 32000])
@pytest.mark.parametrize("form", ["rows", "slots"])
@pytest.mark.parametrize("B", [3, 9])
def test_ticks(hip, B, form, V):
    """B = 3: the single-workgroup tick, a greedy row first and a live min_p row behind it (the workgroup goes from the
    greedy row's early return straight into the next row); B = 9: the smallest wide batch.  Row 1 is stopped (its block is
    garbage); in the slots form the counter ids are not the rows, row 2 ends by its budget; row 0's token is a stop id."""
    L = _lib.lib()
    wide, slots = B > 8, form == "slots"
    D, ring, step0 = 8, 4, 2
    # (the seed: chosen so that the NumPy statement has no draw within 9e-5 of a decision boundary, `_against_the_statement`)
    z, tab, pos, req = _case(V, [0, 1, 4] if B == 3 else [(4 - b) % 5 for b in range(B)], 10 * V + B + (4 if B == 3 else 3))
    pos[1] = -1
    blocks = tab.blocks(range(B))
    blocks[1] = np.array([-1, -1, -1], np.int64)
    ids_of = req if slots else np.arange(B, dtype=np.int32)
    Z, PRM = hip.from_numpy(z), hip.from_numpy(blocks)
    # the reference: the standalone entry (held to the shared entries above) on the same rows
    out = hip.from_numpy(np.full(B, -5, np.int64))
    P0, I0 = hip.from_numpy(pos), hip.from_numpy(ids_of)              # (held until the call has run)
    L.call("pdnq_sample_rows_f32", Z._ptr, V, B, V, PRM._ptr, P0._ptr, I0._ptr, out._ptr, hip.stream())
    want = out.get()
    assert want[1] == -5
    _against_the_statement(z, blocks, pos, ids_of, want)
    stop = np.zeros(-(-V // 32), np.uint32)
    stop[want[0] >> 5] |= np.uint32(1) << np.uint32(want[0] & 31)
    left = np.full(B, 4, np.int32)
    left[1], left[2] = 0, 1
    emb = np.random.default_rng(3).standard_normal((V, D)).astype(f32)
    hist = hip.from_numpy(np.full((ring, B), -7, np.int64))
    hptr = hip.from_numpy(np.array([hist._ptr], np.int64))
    P, ST, R, LF = (hip.from_numpy(a) for a in (pos, np.array([step0], np.int32), req, left))
    AR, STOP = hip.from_numpy(np.zeros(1, np.int32)), hip.from_numpy(stop.view(np.int32))
    ids, E, X = hip.from_numpy(np.full(B, -5, np.int64)), hip.from_numpy(emb), hip.from_numpy(np.full((B, D), 9, f32))
    name = "pdnq_decode%s_sample_tick_%s_f32" % ("_wide" if wide else "", form)
    cnt = (P._ptr, ST._ptr) + ((AR._ptr,) if wide else ())
    slot = (R._ptr, LF._ptr, ring) if slots else ()
    _counters()
    L.call(name, Z._ptr, V, B, V, PRM._ptr, ids._ptr, *cnt, *slot, STOP._ptr, hptr._ptr, E._ptr, D, D, X._ptr, hip.stream())
    c = _counters()
    live = pos >= 0
    got = ids.get()
    assert np.array_equal(got, want)                                    # bit for bit; the stopped row's id untouched
    assert hist.get()[step0].tolist() == [int(t) if l else -1 for t, l in zip(want, live)]
    assert (hist.get()[[0, 1, 3]] == -7).all() and ST.get()[0] == step0 + 1
    hit = np.array([bool((stop[t >> 5] >> np.uint32(t & 31)) & 1) if l else False for t, l in zip(want, live)])
    end = hit | ((left <= 1) if slots else False)
    assert hit[0] and P.get().tolist() == [-1 if (not l or e) else int(p) + 1 for p, l, e in zip(pos, live, end)]
    if slots:
        assert LF.get().tolist() == [int(v) - int(l) for v, l in zip(left, live)]
    x = X.get()
    assert np.array_equal(x[live], emb[want[live]]) and (x[1] == 9).all()
    if wide:
        assert AR.get()[0] == 0
    # counted where the shared form counts, and once in slot 49
    expect = {28: 1, 49: 1, 29: int(not slots or wide), 30: int(slots), 31: int(wide)}
    assert {i: v for i, v in enumerate(c) if v} == {i: v for i, v in expect.items() if v}


# -- end to end ----------------------------------------------------------------------------------------------------
VOCAB = 2500
# request: 0 greedy, 1 T = 0.8, 2 top_k = 5, 3 top_p = 0.9, 4 min_p = 0.1, 5 another seed
MIX = dict(temperature=[0.0, 0.8, 1.0, 1.0, 1.0, 1.0], top_k=[0, 0, 5, 0, 0, 0], top_p=[1.0, 1.0, 1.0, 0.9, 1.0, 1.0],
           min_p=[0.0, 0.0, 0.0, 0.0, 0.1, 0.0], seed=[3, 3, 3, 3, 3, 11])
PEN = dict(repetition_penalty=1.6, presence_penalty=0.8, frequency_penalty=0.3)


def _model(B):
    np.random.seed(8)
    m = Llama(VOCAB, 96, 2, 128, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(VOCAB, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to("hip:0")


def _run(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn()
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _steps(it):
    return np.stack([(t[0] if isinstance(t, tuple) else t).numpy().reshape(-1) for t in it], 1)


def _mix(N):
    kw = {k: [v[r % 6] for r in range(N)] for k, v in MIX.items()}
    return kw, [{k: v[r] for k, v in kw.items()} for r in range(N)]


def _setup(N):
    rng = np.random.default_rng(N)
    return [rng.integers(0, VOCAB, 1 + (7 * r) % 11) for r in range(N)], [3 + (5 * r) % 8 for r in range(N)]


_uniform = {}


def _want(N, **kw):
    """Row r of the uniform generate_ragged run -- request r's values for every row, the same switches and keywords --
    cut to its budget; computed once per (N, keywords, switches) and shared."""
    key = (N, tuple(sorted(kw.items())), Llama.fast_decode)
    if key not in _uniform:
        prompts, budgets = _setup(N)
        sets, rows = _mix(N)[1], {}
        for r, one in enumerate(sets):
            k = tuple(one.items())
            if k not in rows:                          # (request r and r + 6 share a value set: one run)
                m = _model(N)
                rows[k] = _run(m, lambda: _steps(m.generate_ragged(prompts, max(budgets), **one, **kw)))
        _uniform[key] = [rows[tuple(one.items())][r, :budgets[r]].tolist() for r, one in enumerate(sets)]
    return _uniform[key]


def _served(out):
    return [(o[0] if isinstance(o, tuple) else o).tolist() for o in out]


def test_serve_two_slots_on_the_graph_path(hip):
    Graph.clear()
    prompts, budgets = _setup(6)
    want = _want(6)
    assert len({tuple(w[:3]) for w in want}) > 3       # the value sets do differ in what they yield
    m = _model(6)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=2, **_mix(6)[0]))
    st = m._decode_st
    assert _served(got) == want and st["ok"] and st["per_row"] and st["graphs"] and not st["wide"]
    # generate_ragged itself with the table: row r at its own values
    m = _model(6)
    got = _run(m, lambda: _steps(m.generate_ragged(prompts, max(budgets), **_mix(6)[0])))
    assert [g[:b].tolist() for g, b in zip(got, budgets)] == want and m._decode_st["per_row"]
    assert np.array_equal(m._decode_st["params"].get(), S.Table(**_mix(6)[0]).blocks(range(6)))


def test_serve_without_fast_decode(hip, monkeypatch):
    Graph.clear()
    monkeypatch.setattr(Llama, "fast_decode", False)
    prompts, budgets = _setup(6)
    want = _want(6)
    _counters()
    m = _model(6)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=2, **_mix(6)[0]))
    c = _counters()
    assert _served(got) == want and c[49] > 0          # (every draw through the standalone entry)


def test_serve_wide(hip):
    Graph.clear()
    prompts, budgets = _setup(12)
    want = _want(12)
    m = _model(12)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=9, **_mix(12)[0]))
    assert _served(got) == want and m._decode_st["wide"] and m._decode_st["per_row"] and m._decode_st["ok"]


def test_serve_chunked(hip):
    Graph.clear()
    prompts, budgets = _setup(6)
    want = _want(6)
    m = _model(6)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=2, prefill_chunk=4, **_mix(6)[0]))
    assert _served(got) == want and m._decode_st["per_row"] and "mixed" in m._decode_st


def test_speculate(hip):
    Graph.clear()
    prompts, budgets = _setup(6)
    want = _want(6, speculate=2)
    m = _model(6)
    got = _run(m, lambda: _steps(m.generate_ragged(prompts, max(budgets), speculate=2, **_mix(6)[0])))
    assert [g[:b].tolist() for g, b in zip(got, budgets)] == want
    assert m._spec_st["per_row"] and m._spec_st["params"].shape == (6, 3)


def test_with_logprobs_and_a_penalty(hip):
    Graph.clear()
    prompts, budgets = _setup(6)
    want = _want(6, logprobs=2, **PEN)
    m = _model(6)
    got = _run(m, lambda: m.serve_all(prompts, budgets, slots=2, logprobs=2, **PEN, **_mix(6)[0]))
    st = m._decode_st
    assert _served(got) == want and st["per_row"] and st["pen"] and st["lp_n"] == 2 and st["ok"]
    assert all(o[1].top_logprobs.shape == (len(o[0]), 2) and np.isfinite(o[1].token).all() for o in got)


def test_defaults_keep_the_plan_key_and_the_counters(hip):
    """Scalar arguments and min_p = 0: the run of before -- the same plan key, the same counters, no pdnq_ entry."""
    Graph.clear()
    prompts, _ = _setup(5)
    for kw in ({}, dict(temperature=0.9, top_k=40, top_p=0.92, seed=31)):
        m0, m1 = _model(5), _model(5)
        _counters()
        base = _run(m0, lambda: _steps(m0.generate_ragged(prompts, 10, stop_ids=[7], **kw)))
        c0 = _counters()
        Graph.clear()
        again = _run(m1, lambda: _steps(m1.generate_ragged(prompts, 10, stop_ids=[7], min_p=0.0, **kw)))
        c1 = _counters()
        k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
        assert np.array_equal(base, again) and c0 == c1 and c0[49] == 0 and (c0[28] > 0) == bool(kw)
        assert len(k0) == len(k1) == 11 and k0[:5] == k1[:5] and k0[6:] == k1[6:]      # (index 5: the weights' addresses)
        assert m1._decode_st["per_row"] is False and "per_row" not in k1
        Graph.clear()
        _counters()
        a = _run(m0, lambda: _served(m0.serve_all(prompts, 6, slots=2, **kw)))
        c0 = _counters()
        Graph.clear()
        b = _run(m1, lambda: _served(m1.serve_all(prompts, 6, slots=2, min_p=0.0, **kw)))
        c1 = _counters()
        assert a == b and c0 == c1 and c0[49] == 0 and "per_row" not in m1._decode_st["key"]
