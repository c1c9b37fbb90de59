"""Ragged decode on a real MI355X: the per-row-position entries (include/pdn_hip.h, *_rows_f32) against the scalar
entries run one row at a time (bit-exact: the same workgroup code at the same position) and against float64 NumPy
statements of llm/llama/model.py:105-121, the per-row ticks, and `Llama.generate_ragged` end to end on the two-, three-
and five-launch paths, without graphs and on the generic HIP step, against the `cpu` device."""
import math

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


def _rms(x, w, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


def _rope(v, c, s):                          # v (..., H, hd) interleaved pairs
    a = v.reshape(v.shape[:-1] + (v.shape[-1] // 2, 2))
    out = np.empty_like(a)
    out[..., 0] = a[..., 0] * c - a[..., 1] * s
    out[..., 1] = a[..., 0] * s + a[..., 1] * c
    return out.reshape(v.shape)


def _merge(rec, w):
    """(ns, H, 4 + w) softmax partials [m, l, -, - | sum] -> (H, w) merged, in float64."""
    m, l, o = rec[..., 0].astype(np.float64), rec[..., 1].astype(np.float64), rec[..., 4:4 + w].astype(np.float64)
    m = np.where(l > 0, m, -np.inf)
    e = np.where(l > 0, np.exp(m - m.max(0)), 0.0)
    return (e[..., None] * np.where(l[..., None] > 0, o, 0)).sum(0) / (e * l).sum(0)[..., None]


def _positions(rng, B, maxL, kind):
    if kind == "equal":
        return np.full(B, 137 % maxL, np.int32)
    p = rng.integers(1, maxL - 1, B).astype(np.int32)
    p[0] = 0
    if B > 1:
        p[-1] = maxL - 1
    if B > 2:
        p[1] = -1                            # a stopped row
    return p


@pytest.mark.parametrize("kind", ["random", "equal"])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("hd", [48, 64])
@pytest.mark.parametrize("entry", ["block", "oproj", "attention"])
def test_rows_entries(hip, entry, hd, B, kind):
    L = _lib.lib()
    H, maxL, eps = 4, 300, 1e-6
    D = H * hd
    rng = np.random.default_rng(hd * 100 + B + len(kind) + len(entry))
    pos = _positions(rng, B, maxL, kind)
    base = rng.standard_normal((B, D)).astype(f32)
    qkv = rng.standard_normal((B, 3 * D)).astype(f32)
    wqkv = (rng.standard_normal((3, D, D)) / math.sqrt(D)).astype(f32)
    wo = (rng.standard_normal((D, D)) / math.sqrt(D)).astype(f32)
    n1 = (1 + 0.1 * rng.standard_normal(D)).astype(f32)
    kc = rng.standard_normal((B, maxL, H, hd)).astype(f32)
    vc = rng.standard_normal((B, maxL, H, hd)).astype(f32)
    ang = rng.uniform(0, 6.28, (maxL, hd // 2))
    cos, sin = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    dev = {n: hip.from_numpy(a) for n, a in dict(base=base, qkv=qkv, wqkv=wqkv, wo=wo, n1=n1, cos=cos, sin=sin).items()}
    st = hip.stream()
    for ns in range(1, 8):
        if entry == "block" and not (L.query("pdn_decode_block_supported", D, H, hd, ns)
                                     and 0 < L.query("pdn_decode_block_lds_bytes", D, H, hd, ns, maxL) <= 65536):
            continue
        nrec = ns + 1 if entry == "block" else ns
        w = hd if entry == "attention" else D
        R = nrec * H * (4 + w)

        def launch(name, b0, nb, P, K, Vc, out):
            k0, v0, o0 = K._ptr + 4 * b0 * maxL * D, Vc._ptr + 4 * b0 * maxL * D, out._ptr + 4 * b0 * R
            if entry == "block":
                L.call(f"pdn_decode_block_{name}f32", dev["base"]._ptr + 4 * b0 * D, D, None, 0, 0, XO._ptr + 4 * b0 * D,
                       D, dev["n1"]._ptr, eps, dev["wqkv"]._ptr, D, D * D, dev["cos"]._ptr, dev["sin"]._ptr, k0, v0,
                       maxL * D, P._ptr, maxL, dev["wo"]._ptr, D, o0, nb, H, hd, ns, st)
            elif entry == "oproj":
                L.call(f"pdn_decode_attention_oproj_{name}f32", dev["qkv"]._ptr + 4 * b0 * 3 * D, 3 * D, dev["cos"]._ptr,
                       dev["sin"]._ptr, k0, v0, dev["wo"]._ptr, D, o0, nb, H, hd, ns, maxL * D, P._ptr, maxL, st)
            else:
                L.call(f"pdn_decode_attention_{name}f32", dev["qkv"]._ptr + 4 * b0 * 3 * D, 3 * D, dev["cos"]._ptr,
                       dev["sin"]._ptr, k0, v0, o0, nb, H, hd, ns, maxL * D, P._ptr, maxL, st)

        XO = hip.empty((B, D))
        KR, VR, OUT = hip.from_numpy(kc), hip.from_numpy(vc), hip.empty((B, R))
        counters()
        launch("rows_", 0, B, hip.from_numpy(pos), KR, VR, OUT)
        assert counters()[29] == 1
        KS, VS, ONE = hip.from_numpy(kc), hip.from_numpy(vc), hip.empty((B, R))
        for b in np.flatnonzero(pos >= 0):
            launch("", int(b), 1, hip.from_numpy(pos[b:b + 1]), KS, VS, ONE)
        got, one = OUT.get().reshape(B, nrec, H, 4 + w), ONE.get().reshape(B, nrec, H, 4 + w)
        kr, vr, ks, vs = KR.get(), VR.get(), KS.get(), VS.get()
        for b in range(B):
            p = int(pos[b])
            if p < 0:                                                   # a stopped row: its cache is left alone
                assert np.array_equal(kr[b], kc[b]) and np.array_equal(vr[b], vc[b]), (entry, ns, b)
                continue
            assert np.array_equal(kr[b], ks[b]) and np.array_equal(vr[b], vs[b]), (entry, ns, b, "cache slot")
            # [m, l, -, - | sum]: fields 2, 3 are never written; a range without keys is [-inf, 0 | zeros] in every entry
            assert np.array_equal(got[b][..., :2], one[b][..., :2]), (entry, ns, b, "records")
            assert np.array_equal(got[b][..., 4:], one[b][..., 4:]), (entry, ns, b, "records")
            empty = one[b][..., 1] == 0
            assert np.all(got[b][empty][:, 0] == -np.inf) and not got[b][empty][:, 4:].any(), (entry, ns, b, "empty ranges")
            # float64 statement: q (| k | v) of the row, RoPE at its own position, attention over [0, p]
            if entry == "block":
                x = base[b].astype(np.float64)
                q3 = np.einsum("k,jkn->jn", _rms(x, n1, eps), wqkv.astype(np.float64))
            else:
                q3 = qkv[b].astype(np.float64).reshape(3, D)
            c, s_ = cos[p].astype(np.float64), sin[p].astype(np.float64)
            q, k, v = _rope(q3[0].reshape(H, hd), c, s_), _rope(q3[1].reshape(H, hd), c, s_), q3[2].reshape(H, hd)
            K = kc[b, :p + 1].astype(np.float64); K[p] = k
            Vv = vc[b, :p + 1].astype(np.float64); Vv[p] = v
            sc = np.einsum("hd,thd->ht", q, K) / math.sqrt(hd)
            pr = np.exp(sc - sc.max(-1, keepdims=True)); pr /= pr.sum(-1, keepdims=True)
            att = np.einsum("ht,thd->hd", pr, Vv)
            ref = att if entry == "attention" else np.einsum("hd,hdn->hn", att, wo.astype(np.float64).reshape(H, hd, D))
            mer = _merge(got[b], w)
            err = np.abs(mer - ref).max() / np.abs(ref).max()
            assert err < 1e-4, (entry, ns, b, p, err)
            slot = np.stack([k, v])
            err = np.abs(np.stack([kr[b, p], vr[b, p]]) - slot).max() / np.abs(slot).max()
            assert err < 1e-5, (entry, ns, b, p, "appended k / v", err)
            # nothing else of the row's cache moved
            mask = np.ones(maxL, bool); mask[p] = False
            assert np.array_equal(kr[b, mask], kc[b, mask]) and np.array_equal(vr[b, mask], vc[b, mask])


def _history(hip, steps, B):
    buf = hip.from_numpy(np.full((steps, B), -7, np.int64))
    return buf, hip.from_numpy(np.array([buf._ptr], np.int64))


@pytest.mark.parametrize("sampled", [False, True])
def test_rows_ticks(hip, sampled):
    L = _lib.lib()
    B, V, D, n, step = 5, 1000, 96, 40, 3
    rng = np.random.default_rng(7 + sampled)
    z = (3 * rng.standard_normal((B, V))).astype(f32)
    emb = rng.standard_normal((V, D)).astype(f32)
    pos = np.array([4, -1, 11, 0, 30], np.int32)
    if sampled:
        T, k, p_, seed = 0.9, 50, 0.95, 99
        want = np.array([sampling.sample_rows_np(z[b:b + 1], max(int(pos[b]), 0), T, k, p_, seed, rows=[b])[0]
                         for b in range(B)])
    else:
        want = z.argmax(-1)
    stop = np.zeros(-(-V // 32), np.uint32)
    stop[want[2] >> 5] |= np.uint32(1) << np.uint32(want[2] & 31)       # row 2's token stops it
    hist, hptr = _history(hip, 8, B)
    P, S, STOP = hip.from_numpy(pos), hip.from_numpy(np.array([step], np.int32)), hip.from_numpy(stop.view(np.int32))
    ids = hip.from_numpy(np.full(B, 5, np.int64))
    E, X = hip.from_numpy(emb), hip.from_numpy(np.zeros((B, D), f32))
    counters()
    if sampled:
        prm = sampling.params_buffer(T, k, p_, seed)
        Z = hip.from_numpy(z)                              # (kept alive until the launch has read it)
        L.call("pdn_decode_sample_tick_rows_f32", Z._ptr, V, B, V, prm._ptr, ids._ptr, P._ptr, S._ptr,
               STOP._ptr, hptr._ptr, E._ptr, D, D, X._ptr, hip.stream())
    else:
        nb = -(-V // n)
        vals = np.full((B, nb), -np.inf, f32); args = np.zeros((B, nb), np.int32)
        for b in range(B):
            for j in range(nb):
                seg = z[b, j * n:(j + 1) * n]
                vals[b, j], args[b, j] = seg.max(), j * n + int(seg.argmax())
        VA, AR = hip.from_numpy(vals), hip.from_numpy(args)
        L.call("pdn_decode_pick_tick_rows_f32", VA._ptr, AR._ptr, B, nb, ids._ptr,
               P._ptr, S._ptr, STOP._ptr, hptr._ptr, E._ptr, D, D, X._ptr, hip.stream())
    assert counters()[29] == 1
    h, got_ids, p_after, x = hist.get(), ids.get(), P.get(), X.get()
    live = pos >= 0
    tok = h[step]
    if sampled:
        for b in np.flatnonzero(live & (tok != want)):
            assert margin(z[b], int(pos[b]), b, T, k, p_, seed) < 1e-5
    else:
        assert np.array_equal(tok[live], want[live])
    assert tok[1] == -1 and got_ids[1] == 5 and p_after[1] == -1 and not x[1].any()     # the stopped row: left alone
    assert (np.delete(h, step, 0) == -7).all()                                           # only slot `step` written
    assert S.get()[0] == step + 1
    for b in np.flatnonzero(live):
        assert got_ids[b] == tok[b] and np.array_equal(x[b], emb[tok[b]])
        assert p_after[b] == (-1 if tok[b] == want[2] else pos[b] + 1)


def test_attention_decode_rows(hip):
    L = _lib.lib()
    B, H, hd, maxL = 6, 3, 64, 200
    D = H * hd
    rng = np.random.default_rng(3)
    lens = np.array([1, 200, 37, 1, 150, 64], np.int32)
    q = rng.standard_normal((B, D)).astype(f32)
    kc = rng.standard_normal((B, maxL, H, hd)).astype(f32)
    vc = rng.standard_normal((B, maxL, H, hd)).astype(f32)
    Q, K, Vc, O, ONE = (hip.from_numpy(a) for a in (q, kc, vc, np.zeros((B, D), f32), np.zeros((B, D), f32)))
    LENS = hip.from_numpy(lens)
    L.call("pdn_attention_decode_rows_f32", Q._ptr, K._ptr, Vc._ptr, O._ptr, B, H, LENS._ptr,
           int(lens.max()), hd, maxL * D, hip.stream())
    for b in range(B):
        L.call("pdn_attention_decode_f32", Q._ptr + 4 * b * D, K._ptr + 4 * b * maxL * D, Vc._ptr + 4 * b * maxL * D,
               ONE._ptr + 4 * b * D, 1, H, int(lens[b]), hd, maxL * D, hip.stream())
    got = O.get()
    assert np.array_equal(got, ONE.get())
    for b in range(B):
        T = int(lens[b])
        s = np.einsum("hd,thd->ht", q[b].reshape(H, hd).astype(np.float64), kc[b, :T]) / math.sqrt(hd)
        p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
        ref = np.einsum("ht,thd->hd", p, vc[b, :T]).reshape(D)
        assert np.abs(got[b] - ref).max() / np.abs(ref).max() < 1e-4


# -- end to end -------------------------------------------------------------------------------------------------
def _model(dev, B, H=2):
    np.random.seed(8)
    m = Llama(256, 96, H, 128, 64, B, 2, np.float32)
    m.tok_embedding.weight.data[...] = np.random.randn(256, 96).astype(np.float32)
    m.lm_head.weight.data[...] *= 6.0
    return m.to(dev) if dev != "cpu" else m


def _ragged(m, prompts, n, record=None, **kw):
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
            return np.stack([t.numpy().reshape(-1) for t in m.generate_ragged(prompts, n, **kw)], 1)
    finally:
        if record is not None:
            del m.lm_head.forward
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


def _check(got, want, logits, lens, kw):
    if not kw:
        assert np.array_equal(got, want)
        return
    for b in range(got.shape[0]):
        bad = np.flatnonzero(got[b] != want[b])
        if bad.size:                                        # first differing step: its float64 margin must be tiny
            s = int(bad[0])
            mg = margin(logits[s][b], int(lens[b]) + s, b, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0),
                        kw["seed"])
            assert mg < 1e-5, (b, s, mg)


SAMPLED = dict(temperature=0.9, top_p=0.92, seed=31)


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("mode", ["fused2", "fused1", "unfused", "nograph", "generic"])
def test_generate_ragged_on_every_path(hip, mode, kw):
    Graph.clear()
    B = 12 if mode == "generic" else 5
    rng = np.random.default_rng(B + len(kw))
    lens = np.array([1 + (7 * b) % 11 for b in range(B)])
    prompts = [rng.integers(0, 256, n) for n in lens]
    logits = []
    want = _ragged(_model("cpu", B), prompts, 30, record=logits, **kw)
    Llama.fused_decode = {"fused2": 2, "fused1": 1}.get(mode, 0 if mode == "unfused" else 2)
    Llama.graph_decode = mode != "nograph"
    try:
        m = _model("hip:0", B)
        counters()
        got = _ragged(m, prompts, 30, **kw)
        assert counters()[29] > 0
        if mode in ("fused2", "fused1") :
            assert m._decode_st["ragged"] and m._decode_st["graphs"], "no ragged graph captured"
        assert np.array_equal(_ragged(m, prompts, 30, **kw), got)           # reproducible on the same model
    finally:
        Llama.fused_decode, Llama.graph_decode = 2, True
    _check(got, want, logits, lens, kw)


def test_equal_lengths_match_generate_and_stop_ids(hip):
    Graph.clear()
    ids = np.random.default_rng(1).integers(0, 256, (4, 6))
    m = _model("hip:0", 4)
    m.eval()
    with pdn.no_grad():
        rect = np.concatenate([t.numpy() for t in m.generate(ids, 6 + 24)], 1)
    m.train(True)
    pdn.autograd.set_grad_enabled(True)
    counters()
    assert np.array_equal(_ragged(_model("hip:0", 4), list(ids), 24), rect)
    assert counters()[29] > 0
    # stop ids on the graph path: rows stop at their first stop id, yield -1 after, leave their cache alone
    stop = {int(rect[0, 4]), int(rect[2, 9])}
    m = _model("hip:0", 4)
    k0 = [l.attention.cache_k.numpy() for l in m.layers]
    got = _ragged(m, list(ids), 24, stop_ids=stop)
    ends = [next((i for i in range(24) if rect[b, i] in stop), 23) for b in range(4)]
    assert got.shape[1] == max(ends) + 1
    for b in range(4):
        assert np.array_equal(got[b, :ends[b] + 1], rect[b, :ends[b] + 1]) and (got[b, ends[b] + 1:] == -1).all()
        for l, k in zip(m.layers, k0):
            assert np.array_equal(l.attention.cache_k.numpy()[b, 6 + ends[b] + 1:], k[b, 6 + ends[b] + 1:])


def test_rectangular_generate_never_uses_the_rows_entries(hip):
    Graph.clear()
    Llama.graph_decode = False
    try:
        m = _model("hip:0", 3)
        m.eval()
        counters()
        with pdn.no_grad():
            for _ in m.generate(np.array([[1, 2, 3]] * 3), 20):
                pass
        c = counters()
        assert c[29] == 0 and c[28] == 0
    finally:
        Llama.graph_decode = True
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
