"""Speculative decoding on a real MI355X: pdn_spec_draft_rows against the statement of llm/speculative.py, the verify
ticks against float64 NumPy and the wide sample tick, two replays of a pass, and `generate_ragged(speculate=k)` end to end
against the `cpu` reference under the first-difference margin rule of tests/test_serve_gpu.py."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.llm.sampling import params_bytes
from tests.abi_emulator import counters, draft_np, settle_np
from tests.test_serve_gpu import SAMPLED, _check, _model, _ragged_reference

pytestmark = pytest.mark.gpu
f32 = np.float32


def _histories(B, hw, k, seed):
    """Random histories over a small alphabet (many n-gram matches), with dead rows, a row of one token, a row whose
    budget allows no draft and a full row."""
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 5, (B, hw)).astype(np.int32)
    hlen = rng.integers(1, hw + 1, B).astype(np.int32)
    pos = (hlen + rng.integers(0, 3, B)).astype(np.int32)
    left = rng.integers(1, 2 * k + 2, B).astype(np.int32)
    pos[::7] = -1
    for b, (a, v) in enumerate(((hlen, hlen[0]), (hlen, 1), (left, 1), (hlen, hw))):
        if b < B:
            a[b] = v
    return hist, hlen, pos, left


@pytest.mark.parametrize("B,k,hw", [(1, 4, 16), (13, 3, 64), (64, 1, 300), (16, 16, 2048)])
def test_draft_rows_equal_the_statement(hip, B, k, hw):
    L = _lib.lib()
    hist, hlen, pos, left = _histories(B, hw, k, B + k)
    R = B * (k + 1)
    H, HL, P, LF = (hip.from_numpy(a) for a in (hist, hlen, pos, left))
    tok, qpos, runs = (hip.from_numpy(np.full(R, 77, np.int64)), hip.from_numpy(np.full(R, 77, np.int32)),
                       hip.from_numpy(np.full((B, 4), 77, np.int32)))
    counters()
    L.call("pdn_spec_draft_rows", H._ptr, hw, HL._ptr, P._ptr, LF._ptr, B, k, tok._ptr, qpos._ptr, runs._ptr, hip.stream())
    hip.synchronize()
    assert counters()[34] == 1
    t, q, r = draft_np(hist, hlen, pos, left, k)
    assert np.array_equal(qpos.get(), q) and np.array_equal(runs.get(), r)
    assert np.array_equal(tok.get()[q >= 0], t[q >= 0])


def _tick_state(B, k, seed, V):
    rng = np.random.default_rng(seed)
    hw = 64
    hist = rng.integers(0, V, (B, hw)).astype(np.int32)
    hlen = rng.integers(2, 20, B).astype(np.int32)
    pos = (hlen + 1).astype(np.int32)
    pos[B // 2] = -1
    left = rng.integers(1, 2 * k + 2, B).astype(np.int32)
    tok, qpos, _ = draft_np(hist, hlen, pos, left, k)
    return hw, hist, hlen, pos, left, tok, qpos


def _settle(hip, entry, args, B, k, state, stops, V):
    hw, hist, hlen, pos, left, tok, qpos = state
    R = B * (k + 1)
    stops = np.asarray(stops, np.int64)
    mask = np.zeros(-(-V // 32), np.uint32)
    np.bitwise_or.at(mask, stops >> 5, np.uint32(1) << (stops & 31).astype(np.uint32))
    dev = [hip.from_numpy(a) for a in (tok, qpos, np.zeros(R, np.int64), hist, hlen, pos, left, mask.view(np.int32),
                                       np.zeros(1, np.int32))]
    box = hip.Mailbox(1, (B, k + 4), unset=np.iinfo(np.int64).min)
    bp = hip.from_numpy(np.array([box._ptr], np.int64))
    T, Q, PK, H, HL, P, LF, S, ST = dev
    _lib.lib().call(entry, *args, T._ptr, Q._ptr, B, k, PK._ptr, H._ptr, hw, HL._ptr, P._ptr, LF._ptr, S._ptr, ST._ptr,
                    bp._ptr, hip.stream())
    out = np.array(box.slot(0).get())
    hip.synchronize()
    return PK.get(), out, (H.get(), HL.get(), P.get(), LF.get(), ST.get())


def test_pick_tick_equals_the_float64_argmax(hip):
    B, k, V, nblk = 9, 3, 1000, 8
    state = _tick_state(B, k, 1, V)
    R = B * (k + 1)
    rng = np.random.default_rng(2)
    logits = rng.standard_normal((R, V)).astype(f32)
    logits[:, 7] = logits[:, 3]                                      # (a tie: the lower index wins)
    logits[::3, 3] = logits.max(-1)[::3] + 1
    # block candidates as mode 2 of the wide product leaves them: each block's max and its first index
    blk = np.split(np.arange(V), nblk)
    cv = np.stack([logits[:, b].max(-1) for b in blk], 1).astype(f32)
    ci = np.stack([b[logits[:, b].argmax(-1)] for b in blk], 1).astype(np.int32)
    CV, CI = hip.from_numpy(cv), hip.from_numpy(ci)
    stops = [int(logits[5].argmax())]
    picks, out, st = _settle(hip, "pdn_spec_verify_pick_tick_f32", (CV._ptr, CI._ptr, nblk), B, k, state, stops, V)
    hw, hist, hlen, pos, left, tok, qpos = state
    want = logits.astype(np.float64).argmax(-1)
    live = qpos >= 0
    assert np.array_equal(picks[live], want[live])
    h, hl, p, lf = hist.copy(), hlen.astype(np.int64), pos.astype(np.int64), left.astype(np.int64)
    slot = settle_np(tok, qpos, picks, k, h, hl, p, lf, stops)
    assert np.array_equal(out, slot)
    assert np.array_equal(st[1], hl) and np.array_equal(st[2], p) and np.array_equal(st[3], lf) and st[4][0] == 1
    assert np.array_equal(st[0], h)


def test_pick_tick_accepts_drafts_and_stops(hip):
    """Picks set by hand against drafts that exist: everything accepted, one accepted, a stop id inside the accepted
    prefix, a stop id as the bonus token, a dead row."""
    B, k, V = 5, 3, 128
    hist = np.zeros((B, 64), np.int32)
    for b in range(B):
        hist[b, :8] = np.array([1, 2, 3, 4, 5, 1, 2, 3]) + 10 * b      # draft of row b: (4, 5, 1) + 10 b
    hlen = np.full(B, 8, np.int32)
    pos = np.array([9, 9, 9, 9, -1], np.int32)
    left = np.full(B, 10, np.int32)
    tok, qpos, _ = draft_np(hist, hlen, pos, left, k)
    state = (64, hist, hlen, pos, left, tok, qpos)
    want = np.array([[4, 5, 1, 77], [4, 66, 1, 2], [4, 5, 1, 2], [4, 5, 1, 99], [0, 0, 0, 0]]) + 10 * np.arange(B)[:, None]
    want[1, 1], want[3, 3], want[4] = 66, 99, 0
    cv = np.ones((B * (k + 1), 1), f32)
    ci = want.reshape(-1, 1).astype(np.int32)
    CV, CI = hip.from_numpy(cv), hip.from_numpy(ci)
    stops = [25, 99]
    picks, out, st = _settle(hip, "pdn_spec_verify_pick_tick_f32", (CV._ptr, CI._ptr, 1), B, k, state, stops, V)
    live = qpos >= 0
    assert np.array_equal(picks[live], want.reshape(-1)[live])
    assert out[:, :3].tolist() == [[4, 3, 3], [2, 3, 1], [2, 3, 2], [4, 3, 3], [0, 0, 0]]
    assert out[0, 3:].tolist() == [4, 5, 1, 77] and out[2, 3:].tolist() == [24, 25, -1, -1]
    assert out[3, 3:].tolist() == [34, 35, 31, 99] and out[4, 3:].tolist() == [-1] * 4
    h, hl, p, lf = hist.copy(), hlen.astype(np.int64), pos.astype(np.int64), left.astype(np.int64)
    assert np.array_equal(out, settle_np(tok, qpos, picks, k, h, hl, p, lf, stops))
    assert st[2].tolist() == [13, 11, -1, -1, -1] and st[3].tolist() == [6, 8, 8, 6, 10]
    assert np.array_equal(st[0], h) and np.array_equal(st[1], hl)


def test_sample_tick_draws_the_wide_tick_token(hip):
    B, k, V = 6, 2, 3000
    state = _tick_state(B, k, 3, V)
    R = B * (k + 1)
    hw, hist, hlen, pos, left, tok, qpos = state
    logits = (np.random.default_rng(4).standard_normal((R, V)) * 3).astype(f32)
    prm = hip.from_numpy(np.frombuffer(params_bytes(0.8, 0, 0.9, 11), np.int64).copy())
    Z = hip.from_numpy(logits)
    picks, _, _ = _settle(hip, "pdn_spec_verify_sample_tick_f32", (Z._ptr, V, V, prm._ptr), B, k, state, [], V)
    # the wide sample tick on row r alone (one row, counter (qpos[r], its row b) via a one-row batch at row b's slot)
    for r in np.flatnonzero(qpos >= 0):
        b = r // (k + 1)
        rows = np.zeros((b + 1, V), f32)
        rows[b] = logits[r]
        ps = np.full(b + 1, -1, np.int32)
        ps[b] = qpos[r]
        ids, P, Zr = hip.from_numpy(np.zeros((b + 1, 1), np.int64)), hip.from_numpy(ps), hip.from_numpy(rows)
        st, arr = hip.from_numpy(np.zeros(1, np.int32)), hip.from_numpy(np.zeros(1, np.int32))
        _lib.lib().call("pdn_decode_wide_sample_tick_rows_f32", Zr._ptr, V, b + 1, V, prm._ptr, ids._ptr, P._ptr,
                        st._ptr, arr._ptr, None, None, None, 0, 0, None, hip.stream())
        hip.synchronize()
        assert int(ids.get()[b, 0]) == int(picks[r]), r


def _spec_run(m, prompts, n, k, **kw):
    m.eval()
    try:
        with pdn.no_grad():
            got = np.stack([t.numpy().reshape(-1).copy() for t in m.generate_ragged(prompts, n, speculate=k, **kw)], 1)
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
    return got, dict(m.last_speculation)


def _repetitive(lens, seed, period=6):
    rng = np.random.default_rng(seed)
    return [np.resize(rng.integers(0, 256, period), n) for n in lens]


@pytest.mark.parametrize("B,k,lens,stop,kw", [(1, 4, [12], False, {}), (5, 2, [3, 9, 1, 14, 6], True, {}),
                                              (32, 3, None, False, {}), (4, 3, [5, 11, 2, 8], True, SAMPLED)])
def test_end_to_end_against_cpu(hip, B, k, lens, stop, kw):
    Graph.clear()
    lens = lens or [1 + (7 * i) % 17 for i in range(B)]
    prompts = _repetitive(lens, B + k)
    n = 30
    ref, logits = _ragged_reference(prompts, [n] * B, **kw)
    stops = {int(ref[0, 6]), int(ref[B - 1, 9])} if stop else set()
    m = _model("hip:0", max(B, 8))
    counters()
    got, c = _spec_run(m, prompts, n, k, stop_ids=sorted(stops), **kw)
    cnt = counters()
    rows = [g[g >= 0] for g in got]
    _check(rows, ref, logits, prompts, [n] * B, stops, kw)
    assert cnt[34] > 0 and m._spec_st is not None and m._spec_st["graph"], cnt[29:]
    if not kw:
        # greedy: the same tokens as the `cpu` statement run, hence the same counts (they follow from the tokens)
        want, wc = _spec_run(_model("cpu", max(B, 8)), prompts, n, k, stop_ids=sorted(stops))
        assert np.array_equal(got, want)
        assert c == wc
        if wc["passes"] < wc["tokens"]:
            assert c["passes"] < c["tokens"]
        if B == 1:
            assert wc["passes"] < wc["tokens"], wc                 # (the repeated prompt is predicted)


def _long_model(dev, B):
    """The model of tests/test_serve_gpu.py with max_seq_len 320: caches past 256 keys, so 4 key ranges per head."""
    np.random.seed(8)
    m = Llama(256, 96, 2, 128, 320, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(256, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to(dev) if dev != "cpu" else m


def test_end_to_end_long_cache(hip):
    """Rows that cross position 256 on a 320-slot cache (key ranges ns = 4, run lengths d + 1 up to 5) against the
    `cpu` statement run."""
    Graph.clear()
    prompts = _repetitive([250, 40, 261], 17)
    n = 40
    want, wc = _spec_run(_long_model("cpu", 3), prompts, n, 4)
    m = _long_model("hip:0", 3)
    counters()
    got, c = _spec_run(m, prompts, n, 4)
    cnt = counters()
    assert m._spec_st["ns"] == 4 and m._spec_st["graph"] and cnt[34] > 0
    assert np.array_equal(got, want), [np.flatnonzero(g != w)[:3] for g, w in zip(got, want)]
    assert c == wc and wc["drafted"] > 0


def test_two_replays_give_the_same_bits(hip):
    """The captured pass replayed twice from the same row state leaves the same logits and the same picks."""
    Graph.clear()
    prompts = _repetitive([7, 4, 12], 9)
    m = _model("hip:0", 8)
    _spec_run(m, prompts, 4, 3)
    st = m._spec_st
    keep = {n: st[n].copy() for n in ("hist", "hlen", "pos", "left", "step")}
    st["pos"][...] = np.array([8, 5, 13], np.int32)
    st["left"][...] = np.array([9, 9, 9], np.int32)
    for nm in ("pos", "left"):
        keep[nm] = st[nm].copy()
    box = hip.Mailbox(2, (3, 7), unset=np.iinfo(np.int64).min)
    st["mbox_ptr"][...] = np.int64(box._ptr)
    outs = []
    for _ in range(2):
        for nm, v in keep.items():
            st[nm][...] = v
        st["step"][...] = np.int32(0)
        st["graph"].replay()
        hip.synchronize()
        outs.append((st["cand_v"].get().copy(), st["picks"].get().copy(), np.array(box.slot(0).get())))
        box.host[...] = box.unset
    assert all(np.array_equal(a, b) for a, b in zip(*outs))
