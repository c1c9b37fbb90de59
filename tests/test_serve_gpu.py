"""Continuous batching on a real MI355X: the slot ticks (pdn_decode_pick_tick_slots_f32 / pdn_decode_sample_tick_slots_f32)
and pdn_kv_store_slots_f32 against NumPy statements, and `Llama.serve` end to end on the two-, three- and five-launch
paths, without graphs, on the generic HIP step and on the module path, against the `cpu` device."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, margin

pytestmark = pytest.mark.gpu
f32 = np.float32


def _history(hip, steps, B):
    buf = hip.from_numpy(np.full((steps, B), -7, np.int64))
    return buf, hip.from_numpy(np.array([buf._ptr], np.int64))


@pytest.mark.parametrize("step", [2, 9])                          # 9: past the 4-slot ring, slot 9 % 4 = 1
@pytest.mark.parametrize("sampled", [False, True])
def test_slot_ticks(hip, sampled, step):
    L = _lib.lib()
    B, V, D, n, ring = 6, 1000, 96, 40, 4
    rng = np.random.default_rng(7 + sampled + step)
    z = (3 * rng.standard_normal((B, V))).astype(f32)
    emb = rng.standard_normal((V, D)).astype(f32)
    pos = np.array([4, -1, 11, 0, 30, 7], np.int32)              # row 1: empty / stopped
    req = np.array([17, 3, 0, 40, 2, 9], np.int32)               # counter ids: not the rows
    left = np.array([5, 0, 3, 1, 2, 4], np.int32)                # row 3 ends by its budget
    T, k, p_, seed = 0.9, 50, 0.95, 99
    if sampled:
        want = np.array([sampling.sample_rows_np(z[b:b + 1], max(int(pos[b]), 0), T, k, p_, seed, rows=[int(req[b])])[0]
                         for b in range(B)])
    else:
        want = z.argmax(-1)
    stop = np.zeros(-(-V // 32), np.uint32)
    stop[want[2] >> 5] |= np.uint32(1) << np.uint32(want[2] & 31)       # row 2's token stops it
    hist, hptr = _history(hip, ring, B)
    P, S = hip.from_numpy(pos), hip.from_numpy(np.array([step], np.int32))
    R, LF, STOP = hip.from_numpy(req), hip.from_numpy(left), hip.from_numpy(stop.view(np.int32))
    ids = hip.from_numpy(np.full(B, 5, np.int64))
    E, X = hip.from_numpy(emb), hip.from_numpy(np.zeros((B, D), f32))
    counters()
    if sampled:
        prm = sampling.params_buffer(T, k, p_, seed)
        Z = hip.from_numpy(z)
        L.call("pdn_decode_sample_tick_slots_f32", Z._ptr, V, B, V, prm._ptr, ids._ptr, P._ptr, S._ptr, R._ptr, LF._ptr,
               ring, STOP._ptr, hptr._ptr, E._ptr, D, D, X._ptr, hip.stream())
    else:
        nb = -(-V // n)
        vals = np.full((B, nb), -np.inf, f32); args = np.zeros((B, nb), np.int32)
        for b in range(B):
            for j in range(nb):
                seg = z[b, j * n:(j + 1) * n]
                vals[b, j], args[b, j] = seg.max(), j * n + int(seg.argmax())
        VA, AR = hip.from_numpy(vals), hip.from_numpy(args)
        L.call("pdn_decode_pick_tick_slots_f32", VA._ptr, AR._ptr, B, nb, ids._ptr, P._ptr, S._ptr, None, LF._ptr, ring,
               STOP._ptr, hptr._ptr, E._ptr, D, D, X._ptr, hip.stream())
    c = counters()
    assert c[30] == 1 and c[29] == 0 and c[28] == int(sampled)
    h, got_ids, p_after, l_after, x = hist.get(), ids.get(), P.get(), LF.get(), X.get()
    live = pos >= 0
    tok = h[step % ring]
    if sampled:
        for b in np.flatnonzero(live & (tok != want)):
            assert margin(z[b], int(pos[b]), int(req[b]), T, k, p_, seed) < 1e-5
    else:
        assert np.array_equal(tok[live], want[live])
    # the empty row: -1 in the history, everything else left alone
    assert tok[1] == -1 and got_ids[1] == 5 and p_after[1] == -1 and l_after[1] == 0 and not x[1].any()
    assert (np.delete(h, step % ring, 0) == -7).all()                    # only slot step % ring written
    assert S.get()[0] == step + 1
    assert np.array_equal(R.get(), req)
    for b in np.flatnonzero(live):
        assert got_ids[b] == tok[b] and np.array_equal(x[b], emb[tok[b]])
        assert l_after[b] == left[b] - 1
        ends = tok[b] == want[2] or left[b] == 1
        assert p_after[b] == (-1 if ends else pos[b] + 1), b
    assert p_after[3] == -1 and p_after[2] == -1


@pytest.mark.parametrize("D", [96, 288, 30])                      # 30: not a multiple of 4 (the scalar copy)
def test_kv_store_slots(hip, D):
    L = _lib.lib()
    rng = np.random.default_rng(D)
    n_t, A, Ls, Bc, T = 5, 3, 21, 6, 40
    src = [rng.standard_normal((A, Ls, D)).astype(f32) for _ in range(n_t)]
    dst = [rng.standard_normal((Bc, T, D)).astype(f32) for _ in range(n_t)]
    slots = np.array([4, 0, 2], np.int32)
    lens = np.array([21, 1, 13], np.int32)
    S = [hip.from_numpy(a) for a in src]
    Dd = [hip.from_numpy(a) for a in dst]
    stab = hip.from_numpy(np.array([a._ptr for a in S], np.int64))
    dtab = hip.from_numpy(np.array([a._ptr for a in Dd], np.int64))
    SL, LN = hip.from_numpy(slots), hip.from_numpy(lens)
    counters()
    L.call("pdn_kv_store_slots_f32", stab._ptr, Ls * D, dtab._ptr, T * D, n_t, A, Ls, D, SL._ptr, LN._ptr, None, Bc, T,
           hip.stream())
    # a zero row at position lens[i] through the start offsets and a source of batch stride 0
    Z = hip.from_numpy(np.zeros(D, f32))
    ztab = hip.from_numpy(np.full(n_t, Z._ptr, np.int64))
    ONE = hip.from_numpy(np.ones(A, np.int32))
    L.call("pdn_kv_store_slots_f32", ztab._ptr, 0, dtab._ptr, T * D, n_t, A, 1, D, SL._ptr, ONE._ptr, LN._ptr, Bc, T,
           hip.stream())
    assert counters()[30] == 2
    for j in range(n_t):
        want = dst[j].copy()
        for i in range(A):
            want[slots[i], :lens[i]] = src[j][i, :lens[i]]
            want[slots[i], lens[i]] = 0
        assert np.array_equal(Dd[j].get(), want), j                       # bit-exact; pads and other rows untouched


def test_kv_store_slots_clamps_to_the_cache(hip):
    L = _lib.lib()
    D, T = 64, 16
    src = np.random.default_rng(1).standard_normal((2, 20, D)).astype(f32)
    dst = np.zeros((3, T, D), f32)
    S, Dd = hip.from_numpy(src), hip.from_numpy(dst)
    stab, dtab = hip.from_numpy(np.array([S._ptr], np.int64)), hip.from_numpy(np.array([Dd._ptr], np.int64))
    SL, LN = hip.from_numpy(np.array([1, 7], np.int32)), hip.from_numpy(np.array([20, 5], np.int32))   # row 7: outside
    L.call("pdn_kv_store_slots_f32", stab._ptr, 20 * D, dtab._ptr, T * D, 1, 2, 20, D, SL._ptr, LN._ptr, None, 3, T,
           hip.stream())
    got = Dd.get()
    assert np.array_equal(got[1], src[0, :T]) and not got[0].any() and not got[2].any()


# -- end to end -------------------------------------------------------------------------------------------------
def _model(dev, B, H=2):
    np.random.seed(8)
    m = Llama(256, 96, H, 128, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(256, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to(dev) if dev != "cpu" else m


def _serve_all(m, prompts, budgets, record=None, **kw):
    m.eval()
    fwd = m.lm_head.forward
    if record is not None:
        def rec(x):
            y = fwd(x)
            record.append(np.asarray(y.numpy())[:, -1, :])
            return y
        m.lm_head.forward = rec
    try:
        with pdn.no_grad():
            return m.serve_all(prompts, budgets, **kw)
    finally:
        if record is not None:
            del m.lm_head.forward
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _ragged_reference(prompts, budgets, **kw):
    """generate_ragged over every request on the `cpu` device, with every step's logits (row r = request r)."""
    m = _model("cpu", len(prompts))
    seen = []
    fwd = m.lm_head.forward

    def rec(x):
        y = fwd(x)
        seen.append(np.asarray(y.numpy())[:, -1, :])
        return y
    m.lm_head.forward = rec
    m.eval()
    try:
        with pdn.no_grad():
            toks = np.stack([t.numpy().reshape(-1) for t in m.generate_ragged(prompts, int(max(budgets)), **kw)], 1)
    finally:
        del m.lm_head.forward
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
    return toks, seen


def _check(got, ref, logits, prompts, budgets, stops, kw):
    """The first token that differs from the reference must sit at a float64 margin below 1e-5; up to it, equal."""
    for r, g in enumerate(got):
        w = ref[r, :budgets[r]].tolist()
        hit = next((i for i, t in enumerate(w) if t in stops), None)
        w = np.array(w if hit is None else w[:hit + 1])
        if np.array_equal(g, w):
            continue
        n = min(len(g), len(w))
        bad = np.flatnonzero(g[:n] != w[:n])
        assert bad.size, (r, g, w)                              # (same prefix, different length: a stop / budget bug)
        s = int(bad[0])
        z = logits[s][r]
        if kw:
            mg = margin(z, len(prompts[r]) + s, r, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw["seed"])
        else:
            srt = np.sort(z.astype(np.float64))
            mg = srt[-1] - srt[-2]
        assert mg < 1e-5, (r, s, mg)


SAMPLED = dict(temperature=0.9, top_p=0.92, seed=31)


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("mode", ["fused2", "fused1", "unfused", "nograph", "generic", "module"])
def test_serve_on_every_path(hip, mode, kw):
    Graph.clear()
    N, slots = (14, 10) if mode == "generic" else (13, 5)          # generic: 10 rows > 8, the plan refuses
    rng = np.random.default_rng(N + len(kw))
    prompts = [rng.integers(0, 256, 1 + (7 * r) % 11) for r in range(N)]
    budgets = [(5 * r) % 23 for r in range(N)]                      # 0 .. 22
    ref, logits = _ragged_reference(prompts, budgets, **kw)
    stops = {int(ref[3, 4]), int(ref[8, 10])}
    Llama.fused_decode = {"fused2": 2, "fused1": 1}.get(mode, 0 if mode == "unfused" else 2)
    Llama.graph_decode = mode != "nograph"
    Llama.fast_decode = mode != "module"
    try:
        for st in ((), stops):
            m = _model("hip:0", slots)
            counters()
            got = _serve_all(m, prompts, budgets, slots=slots, stop_ids=st, **kw)
            c = counters()
            assert c[30] > 0                                        # (the module path: at least the store)
            if mode in ("fused2", "fused1"):
                assert m._decode_st["serve"] and m._decode_st["graphs"], "no serve graph captured"
            if mode not in ("module",):
                assert c[29] > 0
            assert all(np.array_equal(a, b) for a, b in zip(_serve_all(m, prompts, budgets, slots=slots, stop_ids=st,
                                                                       **kw), got))   # reproducible on the same model
            _check(got, ref, logits, prompts, budgets, st, kw)
    finally:
        Llama.fused_decode, Llama.graph_decode, Llama.fast_decode = 2, True, True


def test_slots_do_not_change_tokens(hip):
    """The same requests through 1, 3 and 8 rows on the graph path: a sampled token depends on its request, not its row."""
    Graph.clear()
    rng = np.random.default_rng(5)
    prompts = [rng.integers(0, 256, 1 + (3 * r) % 9) for r in range(9)]
    budgets = [4 + (7 * r) % 17 for r in range(9)]
    ref, logits = _ragged_reference(prompts, budgets, **SAMPLED)
    for slots in (1, 3, 8):
        got = _serve_all(_model("hip:0", 8), prompts, budgets, slots=slots, **SAMPLED)
        _check(got, ref, logits, prompts, budgets, set(), SAMPLED)


def test_generate_and_generate_ragged_leave_counter_30_alone(hip):
    Graph.clear()
    m = _model("hip:0", 3)
    m.eval()
    counters()
    try:
        with pdn.no_grad():
            for kw in ({}, SAMPLED):
                for _ in m.generate(np.array([[1, 2, 3]] * 3), 20, **kw):
                    pass
                for _ in m.generate_ragged([[1, 2], [3], [4, 5, 6]], 15, stop_ids=[7], **kw):
                    pass
        c = counters()
        assert c[30] == 0 and c[29] > 0
        assert not m._decode_st["serve"]
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
