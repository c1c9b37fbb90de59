"""The wide decode step (csrc/decode_wide.hip, 9 .. 256 rows) on a real MI355X: the MFMA product with every load mode
and epilogue against float64 NumPy, the workgroup-per-row ticks against NumPy statements and against the single-workgroup
slot tick of sample.hip, and `generate` / `generate_ragged` / `serve` end to end against the `cpu` device under the
first-difference margin rule of tests/test_serve_gpu.py."""
import math

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, margin
from tests.test_serve_gpu import _check, _model, _ragged_reference, _serve_all

pytestmark = pytest.mark.gpu
f32 = np.float32
D, H, F, V, EPS = 288, 6, 768, 32000, 1e-5
HD = D // H
COUNTERS = 192                                                    # arrival counters at the start of the workspace


def _rms(x, w):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + EPS) * w


def _merge(rec, ns):
    B = rec.shape[0]
    R = rec.reshape(B, ns, H, 4 + HD)
    m, l, o = R[..., 0], R[..., 1], R[..., 4:]
    w = np.where(l > 0, np.exp(m - np.where(l > 0, m, -np.inf).max(1, keepdims=True)), 0)
    return ((w[..., None] * o).sum(1) / (w * l).sum(1)[..., None]).reshape(B, D)


def _case(name, B, rng):
    """(mode, epi, K, N, input rows, float64 A, W, bias) of one load mode / epilogue case."""
    ns = 3
    if name == "qkv":                                             # RMSNorm in the load, store, three column blocks
        x = rng.standard_normal((B, D)).astype(f32)
        nw = (1 + 0.1 * rng.standard_normal(D)).astype(f32)
        return 1, 0, D, 3 * D, x, nw, _rms(x.astype(np.float64), nw.astype(np.float64)), None
    if name == "oproj":                                           # merge of key-range partials, residual add
        rec = rng.standard_normal((B, ns, H, 4 + HD)).astype(f32)
        rec[..., 1] = rng.uniform(0.5, 3.0, (B, ns, H))
        rec[:, 2, 1, 1] = 0.0                                     # a range with no keys for head 1
        return 3, 1, D, D, rec.reshape(B, -1), None, _merge(rec.astype(np.float64), ns), None
    if name == "gateup":
        x = rng.standard_normal((B, D)).astype(f32)
        nw = (1 + 0.1 * rng.standard_normal(D)).astype(f32)
        return 1, 0, D, 2 * F, x, nw, _rms(x.astype(np.float64), nw.astype(np.float64)), None
    if name == "down":                                            # SwiGLU in the load, residual add
        gu = rng.standard_normal((B, 2 * F)).astype(f32)
        g, u = gu[:, :F].astype(np.float64), gu[:, F:].astype(np.float64)
        return 2, 1, F, D, gu, None, g / (1 + np.exp(-g)) * u, None
    if name == "vocab":                                           # RMSNorm, bias, candidates
        x = rng.standard_normal((B, D)).astype(f32)
        nw = (1 + 0.1 * rng.standard_normal(D)).astype(f32)
        return 1, 2, D, V, x, nw, _rms(x.astype(np.float64), nw.astype(np.float64)), rng.standard_normal(V).astype(f32)
    x = rng.standard_normal((B, 96)).astype(f32)                  # "odd": plain, a width that is not a tile multiple
    return 0, 0, 96, 100, x, None, x.astype(np.float64), rng.standard_normal(100).astype(f32)


def _launch(hip, mode, epi, K, N, X, nw, Wt, blk, bias, Y, CV, CI, P, B, work, ns=3):
    _lib.lib().call("pdn_decode_wide_gemm_f32", X._ptr, X.shape[1], mode, nw._ptr if nw is not None else None, EPS, ns, HD,
                    Wt._ptr, blk, blk, K * blk, bias._ptr if bias is not None else None, Y._ptr, N, epi,
                    CV._ptr if CV is not None else None, CI._ptr if CI is not None else None,
                    P._ptr if P is not None else None, B, K, N, work._ptr if work is not None else None, hip.stream())


@pytest.mark.parametrize("B", [9, 16, 31, 64, 200, 256])
@pytest.mark.parametrize("name", ["qkv", "oproj", "gateup", "down", "vocab", "odd"])
def test_wide_gemm_against_float64(hip, name, B):
    rng = np.random.default_rng(B * 7 + len(name))
    mode, epi, K, N, x, nw, A, bias = _case(name, B, rng)
    blk = {"qkv": D, "gateup": F}.get(name, N)                   # column blocks of the stacked q | k | v, gate | up
    W = (rng.standard_normal((N // blk, K, blk)) / math.sqrt(K)).astype(f32)
    Wfull = np.concatenate(list(W), axis=1).astype(np.float64)
    y0 = rng.standard_normal((B, N)).astype(f32)
    pos = np.arange(B, dtype=np.int32) + 3
    pos[[1, B // 2]] = -1                                         # stopped rows: not computed, y left alone
    want = A @ Wfull + (bias if bias is not None else 0)
    bound = np.abs(A) @ np.abs(Wfull) * 2e-6 + 1e-6
    if epi == 1:
        want = want + y0
        bound = bound + np.abs(y0) * 1e-7
    nb = _lib.lib().query("pdn_decode_wide_blocks", N)
    wf = _lib.lib().query("pdn_decode_wide_work_floats", B, K, N)
    work = hip.from_numpy(np.zeros(max(wf, 4), f32))
    X, Wt, P = hip.from_numpy(x), hip.from_numpy(W), hip.from_numpy(pos)
    nwb = hip.from_numpy(nw) if nw is not None else None
    bb = hip.from_numpy(bias) if bias is not None else None
    outs = []
    for _ in range(2):                                            # two launches: the same bits
        Y = hip.from_numpy(y0)
        CV = hip.from_numpy(np.zeros((B, nb), f32)) if epi == 2 else None
        CI = hip.from_numpy(np.zeros((B, nb), np.int32)) if epi == 2 else None
        counters()
        _launch(hip, mode, epi, K, N, X, nwb, Wt, blk, bb, Y, CV, CI, P, B, work)
        assert counters()[31] == 1
        outs.append((Y.get(), CV.get() if CV is not None else None, CI.get() if CI is not None else None))
    got, cv, ci = outs[0]
    assert np.array_equal(outs[0][0], outs[1][0]) and (cv is None or (np.array_equal(cv, outs[1][1])
                                                                       and np.array_equal(ci, outs[1][2])))
    assert not work.get()[:COUNTERS].any() or wf == 0             # (every arrival counter is back at zero)
    live = pos >= 0
    assert np.array_equal(got[~live], y0[~live])
    err = np.abs(got[live] - want[live])
    assert (err <= bound[live]).all(), float((err - bound[live]).max())
    if epi == 2:
        for b in np.flatnonzero(live):
            j = int(np.argmax(cv[b]))                             # (the pick tick's finish: first maximum of the blocks)
            t = int(ci[b, j])
            assert want[b, t] >= want[b].max() - 2 * bound[b].max(), (b, t)
            assert cv[b, j] == got[b, t]


@pytest.mark.parametrize("B", [16, 64])
@pytest.mark.parametrize("Dm,Hm,Fm", [(512, 8, 1376), (768, 12, 2048)])     # the stories42M / stories110M widths
def test_split_products_share_one_workspace(hip, Dm, Hm, Fm, B):
    """The four products of a layer, twice over, on ONE workspace (as a decode step runs them): shapes whose split
    counts and tile counts differ must not disturb each other's arrival counters."""
    L = _lib.lib()
    rng = np.random.default_rng(Dm + B)
    hd, ns = Dm // Hm, 2
    shapes = []                                                   # (mode, epi, K, N, blk, x, A float64, norm weight)
    x = rng.standard_normal((B, Dm)).astype(f32)
    nw = (1 + 0.1 * rng.standard_normal(Dm)).astype(f32)
    A = x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).mean(-1, keepdims=True) + EPS) * nw
    shapes.append((1, 0, Dm, 3 * Dm, Dm, x, A, nw))
    rec = rng.standard_normal((B, ns, Hm, 4 + hd)).astype(f32)
    rec[..., 1] = rng.uniform(0.5, 3.0, (B, ns, Hm))
    R = rec.astype(np.float64)
    w = np.exp(R[..., 0] - R[..., 0].max(1, keepdims=True))
    Am = ((w[..., None] * R[..., 4:]).sum(1) / (w * R[..., 1]).sum(1)[..., None]).reshape(B, Dm)
    shapes.append((3, 1, Dm, Dm, Dm, rec.reshape(B, -1), Am, None))
    shapes.append((1, 0, Dm, 2 * Fm, Fm, x, A, nw))
    gu = rng.standard_normal((B, 2 * Fm)).astype(f32)
    g, u = gu[:, :Fm].astype(np.float64), gu[:, Fm:].astype(np.float64)
    shapes.append((2, 1, Fm, Dm, Dm, gu, g / (1 + np.exp(-g)) * u, None))
    wf = max(L.query("pdn_decode_wide_work_floats", B, K, N) for _, _, K, N, *_ in shapes)
    work = hip.from_numpy(np.zeros(wf, f32))
    pos = hip.from_numpy(np.arange(B, dtype=np.int32))
    dev = []
    for mode, epi, K, N, blk, xin, Aw, nwv in shapes:
        W = (rng.standard_normal((N // blk, K, blk)) / math.sqrt(K)).astype(f32)
        y0 = rng.standard_normal((B, N)).astype(f32)
        dev.append((hip.from_numpy(xin), hip.from_numpy(W), hip.from_numpy(nwv) if nwv is not None else None, y0,
                    Aw @ np.concatenate(list(W), axis=1).astype(np.float64),
                    np.abs(Aw) @ np.abs(np.concatenate(list(W), axis=1)).astype(np.float64) * 2e-6 + 1e-6))
    for rnd in range(2):
        for (mode, epi, K, N, blk, *_), (X, Wd, NW, y0, want, bound) in zip(shapes, dev):
            Y = hip.from_numpy(y0)
            L.call("pdn_decode_wide_gemm_f32", X._ptr, X.shape[1], mode, NW._ptr if NW is not None else None, EPS, ns, hd,
                   Wd._ptr, blk, blk, K * blk, None, Y._ptr, N, epi, None, None, pos._ptr, B, K, N, work._ptr, hip.stream())
            got = Y.get()
            ref = want + (y0 if epi == 1 else 0)
            err = np.abs(got - ref) - bound - (np.abs(y0) * 1e-7 if epi == 1 else 0)
            assert (err <= 0).all(), (rnd, mode, N, float(err.max()))
    assert not work.get()[:COUNTERS].any()


@pytest.mark.parametrize("kw", [{}, dict(temperature=0.9, top_p=0.92, seed=31)])
def test_generate_wide_at_stories42m_width(hip, kw):
    """D 512, F 1376: q | k | v, gate | up and the narrow products split differently and share the step's workspace."""
    Graph.clear()
    B = 16

    def model(dev):
        np.random.seed(4)
        m = Llama(256, 512, 8, 1376, 64, B, 2, np.float32)
        m.tok_embedding.weight.data[...] = np.random.randn(256, 512).astype(np.float32)
        m.lm_head.weight.data[...] *= 6.0
        return m.to(dev) if dev != "cpu" else m
    ids = np.random.default_rng(2).integers(0, 256, (B, 4))
    ref_m, seen = model("cpu"), []
    fwd = ref_m.lm_head.forward

    def rec(x):
        y = fwd(x)
        seen.append(np.asarray(y.numpy())[:, -1, :])
        return y
    ref_m.lm_head.forward = rec
    ref = _eval(ref_m, lambda: np.concatenate([np.asarray(t.numpy()) for t in ref_m.generate(ids, 24, **kw)], 1))
    m = model("hip:0")
    counters()
    got = _eval(m, lambda: np.concatenate([np.asarray(t.numpy()) for t in m.generate(ids, 24, **kw)], 1))
    assert m._decode_st["ok"] and m._decode_st["wide"] and counters()[31] > 0
    _check_rect(got, ref, seen, 4, kw)


def _hist(hip, steps, B):
    buf = hip.from_numpy(np.full((steps, B), -7, np.int64))
    return buf, hip.from_numpy(np.array([buf._ptr], np.int64))


@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B", [9, 64, 256])
def test_wide_ticks(hip, sampled, slots, B):
    L = _lib.lib()
    Vt, Dt, ring, step = 1000, 96, 4, 6
    rng = np.random.default_rng(B + 2 * sampled + slots)
    z = (3 * rng.standard_normal((B, Vt))).astype(f32)
    emb = rng.standard_normal((Vt, Dt)).astype(f32)
    pos = rng.integers(0, 50, B).astype(np.int32)
    pos[::5] = -1                                                 # stopped / empty rows
    req = rng.permutation(B).astype(np.int32)
    left = rng.integers(1, 4, B).astype(np.int32)
    T, k, p_, seed = 0.9, 50, 0.95, 123
    cnt = req if slots else np.arange(B)
    if sampled:
        want = np.array([sampling.sample_rows_np(z[b:b + 1], max(int(pos[b]), 0), T, k, p_, seed, rows=[int(cnt[b])])[0]
                         for b in range(B)])
    else:
        want = z.argmax(-1)
    stop = np.zeros(-(-Vt // 32), np.uint32)
    for t in want[1:B:7]:                                         # some rows' tokens stop them
        stop[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    steps = ring if slots else step + 1
    hist, hptr = _hist(hip, steps, B)
    P, S, AR = hip.from_numpy(pos), hip.from_numpy(np.array([step], np.int32)), hip.from_numpy(np.zeros(1, np.int32))
    R, LF, STOP = hip.from_numpy(req), hip.from_numpy(left), hip.from_numpy(stop.view(np.int32))
    ids = hip.from_numpy(np.full(B, 5, np.int64))
    E, X = hip.from_numpy(emb), hip.from_numpy(np.zeros((B, Dt), f32))
    counters()
    if sampled:
        prm, Z = sampling.params_buffer(T, k, p_, seed), hip.from_numpy(z)
        head = (Z._ptr, Vt, B, Vt, prm._ptr)
    else:
        nb = -(-Vt // 32)
        vals, args = np.full((B, nb), -np.inf, f32), np.zeros((B, nb), np.int32)
        for j in range(nb):
            seg = z[:, j * 32:(j + 1) * 32]
            vals[:, j], args[:, j] = seg.max(-1), j * 32 + seg.argmax(-1)
        VA, AA = hip.from_numpy(vals), hip.from_numpy(args)
        head = (VA._ptr, AA._ptr, B, nb)
    kind = "sample" if sampled else "pick"
    tail = (hptr._ptr, E._ptr, Dt, Dt, X._ptr, hip.stream())
    if slots:
        L.call(f"pdn_decode_wide_{kind}_tick_slots_f32", *head, ids._ptr, P._ptr, S._ptr, AR._ptr, R._ptr, LF._ptr, ring,
               STOP._ptr, *tail)
    else:
        L.call(f"pdn_decode_wide_{kind}_tick_rows_f32", *head, ids._ptr, P._ptr, S._ptr, AR._ptr, STOP._ptr, *tail)
    c = counters()
    assert c[31] == 1 and c[29] == 1 and c[30] == int(slots) and c[28] == int(sampled)
    assert S.get()[0] == step + 1 and AR.get()[0] == 0
    h, got_ids, p_after, l_after, x = hist.get(), ids.get(), P.get(), LF.get(), X.get()
    slot = step % ring if slots else step
    tok = h[slot]
    assert (np.delete(h, slot, 0) == -7).all()
    live = pos >= 0
    assert (tok[~live] == -1).all() and (got_ids[~live] == 5).all() and (p_after[~live] == -1).all()
    assert not x[~live].any() and np.array_equal(l_after[~live], left[~live])
    if sampled:
        for b in np.flatnonzero(live & (tok != want)):
            assert margin(z[b], int(pos[b]), int(cnt[b]), T, k, p_, seed) < 1e-5
    else:
        assert np.array_equal(tok[live], want[live])
    for b in np.flatnonzero(live):
        t = tok[b]
        assert got_ids[b] == t and np.array_equal(x[b], emb[t])
        hit = bool((stop[t >> 5] >> np.uint32(t & 31)) & 1)
        if slots:
            assert l_after[b] == left[b] - 1
            hit = hit or left[b] == 1
        assert p_after[b] == (-1 if hit else pos[b] + 1), b


@pytest.mark.parametrize("B", [1, 5, 8])
def test_wide_sample_tick_draws_as_the_slot_tick(hip, B):
    """The same logits and (position, counter id): bit-equal tokens from the one-workgroup slot tick of sample.hip."""
    L = _lib.lib()
    Vt, ring = 3000, 4
    rng = np.random.default_rng(40 + B)
    z = (2 * rng.standard_normal((B, Vt))).astype(f32)
    pos = rng.integers(0, 100, B).astype(np.int32)
    req = rng.integers(0, 1000, B).astype(np.int32)
    prm = sampling.params_buffer(1.1, 200, 0.9, 77)
    Z = hip.from_numpy(z)
    toks = []
    for name, extra in (("pdn_decode_sample_tick_slots_f32", ()), ("pdn_decode_wide_sample_tick_slots_f32", (0,))):
        hist, hptr = _hist(hip, ring, B)
        P, S, ids = hip.from_numpy(pos), hip.from_numpy(np.zeros(1, np.int32)), hip.from_numpy(np.zeros(B, np.int64))
        R, LF = hip.from_numpy(req), hip.from_numpy(np.full(B, 9, np.int32))
        AR = hip.from_numpy(np.zeros(1, np.int32))                     # (held until the tick has run)
        cnt = (P._ptr, S._ptr) + ((AR._ptr,) if extra else ())
        L.call(name, Z._ptr, Vt, B, Vt, prm._ptr, ids._ptr, *cnt, R._ptr, LF._ptr, ring, None, hptr._ptr, None, 0, 0,
               None, hip.stream())
        toks.append(hist.get()[0])
    assert np.array_equal(toks[0], toks[1])


# -- end to end -------------------------------------------------------------------------------------------------
SAMPLED = dict(temperature=0.9, top_p=0.92, seed=31)


def _eval(m, fn):
    m.eval()
    try:
        with pdn.no_grad():
            return fn()
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _generate_reference(ids, total, **kw):
    m = _model("cpu", ids.shape[0])
    seen, fwd = [], m.lm_head.forward

    def rec(x):
        y = fwd(x)
        seen.append(np.asarray(y.numpy())[:, -1, :])
        return y
    m.lm_head.forward = rec
    toks = _eval(m, lambda: np.concatenate([np.asarray(t.numpy()) for t in m.generate(ids, total, **kw)], 1))
    return toks, seen


def _check_rect(got, ref, logits, L, kw):
    for b in range(ref.shape[0]):
        if np.array_equal(got[b], ref[b]):
            continue
        s = int(np.flatnonzero(got[b] != ref[b])[0])
        z = logits[s][b]
        if kw:
            mg = margin(z, L + s, b, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw["seed"])
        else:
            srt = np.sort(z.astype(np.float64))
            mg = srt[-1] - srt[-2]
        assert mg < 1e-5, (b, s, mg)


@pytest.fixture()
def graphs(request):
    Graph.clear()
    Llama.graph_decode = request.param
    yield request.param
    Llama.graph_decode = True


@pytest.mark.parametrize("graphs", [True, False], indirect=True)
@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [9, 16, 64])
def test_generate_wide(hip, graphs, kw, B):
    ids = np.random.default_rng(B).integers(0, 256, (B, 5))
    ref, logits = _generate_reference(ids, 40, **kw)
    m = _model("hip:0", B)
    counters()
    got = _eval(m, lambda: np.concatenate([np.asarray(t.numpy()) for t in m.generate(ids, 40, **kw)], 1))
    c = counters()
    st = m._decode_st
    assert st["ok"] and st["wide"] and c[31] > 0
    assert bool(st["graphs"]) == graphs
    assert np.array_equal(_eval(m, lambda: np.concatenate([np.asarray(t.numpy()) for t in m.generate(ids, 40, **kw)],
                                                          1)), got)            # reproducible on the same model
    _check_rect(got, ref, logits, 5, kw)


@pytest.mark.parametrize("graphs", [True, False], indirect=True)
@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("B", [9, 16, 64])
def test_generate_ragged_and_serve_wide(hip, graphs, kw, B):
    rng = np.random.default_rng(100 + B)
    prompts = [rng.integers(0, 256, 1 + (7 * r) % 13) for r in range(B)]
    budgets = [1 + (5 * r) % 30 for r in range(B)]
    ref, logits = _ragged_reference(prompts, budgets, **kw)
    stops = {int(ref[1, 3]), int(ref[B - 1, 6])}
    m = _model("hip:0", B)
    counters()
    got = _eval(m, lambda: np.stack([np.asarray(t.numpy()).reshape(-1)
                                     for t in m.generate_ragged(prompts, max(budgets), stop_ids=stops, **kw)], 1))
    c = counters()
    assert m._decode_st["ok"] and m._decode_st["wide"] and c[31] > 0 and c[29] > 0
    rows = []
    for r in range(B):
        t = got[r, :budgets[r]]
        t = t[t >= 0]
        rows.append(t)
    _check(rows, ref, logits, prompts, budgets, stops, kw)
    # serve: the same requests and twice as many, through B slots
    counters()
    served = _serve_all(m, prompts, budgets, slots=B, stop_ids=stops, **kw)
    c = counters()
    assert m._decode_st["serve"] and m._decode_st["wide"] and c[31] > 0 and c[30] > 0
    assert bool(m._decode_st["graphs"]) == graphs
    _check(served, ref, logits, prompts, budgets, stops, kw)
    again = _serve_all(m, prompts, budgets, slots=B, stop_ids=stops, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(again, served))


def test_slot_count_does_not_change_sampled_tokens(hip):
    """The same requests through 8, 16 and 64 rows: the B <= 8 plan and the wide step draw the same tokens."""
    Graph.clear()
    rng = np.random.default_rng(9)
    prompts = [rng.integers(0, 256, 1 + (3 * r) % 9) for r in range(64)]
    budgets = [2 + (7 * r) % 19 for r in range(64)]
    outs = [_serve_all(_model("hip:0", 64), prompts, budgets, slots=s, **SAMPLED) for s in (8, 16, 64)]
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(o, outs[0]))


@pytest.mark.parametrize("kw", [{}, SAMPLED])
def test_generic_step_when_wide_decode_is_off(hip, kw):
    Graph.clear()
    B = 12
    rng = np.random.default_rng(12)
    prompts = [rng.integers(0, 256, 1 + (5 * r) % 9) for r in range(B)]
    budgets = [3 + (4 * r) % 15 for r in range(B)]
    ref, logits = _ragged_reference(prompts, budgets, **kw)
    Llama.wide_decode = False
    try:
        m, m2 = _model("hip:0", B), _model("hip:0", B)
        counters()
        got = _serve_all(m, prompts, budgets, slots=B, **kw)
        ids = np.random.default_rng(3).integers(0, 256, (B, 4))
        gen = _eval(m2, lambda: np.concatenate([np.asarray(t.numpy()) for t in m2.generate(ids, 20, **kw)], 1))
        c = counters()
    finally:
        Llama.wide_decode = True
    assert c[31] == 0 and c[29] > 0 and not m._decode_st["ok"] and not m2._decode_st["ok"]
    _check(got, ref, logits, prompts, budgets, set(), kw)
    gref, glog = _generate_reference(ids, 20, **kw)
    _check_rect(gen, gref, glog, 4, kw)
