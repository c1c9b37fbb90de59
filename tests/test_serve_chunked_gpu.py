"""Chunked prefill on a real MI355X: pdn_kv_append_rows_f32 + pdn_decode_extend_attention_f32 followed by the mode-3 merge
of pdn_decode_wide_gemm_f32 against float64 NumPy, and `Llama.serve(prefill_chunk=C)` end to end against the `cpu`
generate_ragged reference under the first-difference margin rule of tests/test_serve_gpu.py."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from tests.abi_emulator import counters, rotate
from tests.test_serve_gpu import SAMPLED, _check, _model, _ragged_reference, _serve_all

pytestmark = pytest.mark.gpu
f32 = np.float32


def _layout(max_len, C):
    """Runs per cache row [q0, n, start, ends] over 8 cache rows: decode runs, a run from 0, one across the 256-key range
    boundary, one that ends at the cache's last position, a row outside the layout."""
    S = 8
    runs = [(None, 1, 37, 0), (None, 0, 0, 0), (None, 20, 0, 1), (None, 1, 300, 0), (None, 30, 250, 1),
            (None, 17, max_len - 17, 1), (None, 1, 0, 0), (None, 5, 100, 0)]
    out, q = [], S
    for r, (_, n, s0, e) in enumerate(runs):
        if n == 1:
            out.append((r, 1, s0, 0))
        elif n == 0:
            out.append((0, 0, 0, 0))
        else:
            out.append((q, n, s0, e))
            q += n
    assert q - S <= C
    return np.array(out, np.int32), S + C


@pytest.mark.parametrize("H,hd", [(6, 48), (4, 64), (8, 64)])
@pytest.mark.parametrize("ns", [1, 4])
def test_extend_attention_and_merge(hip, H, hd, ns):
    L = _lib.lib()
    D, max_len, C, rows = H * hd, 320, 80, 8
    runs, nq = _layout(max_len, C)
    rng = np.random.default_rng(H + hd + ns)
    qkv = rng.standard_normal((nq, 3 * D)).astype(f32)
    kc = rng.standard_normal((rows, max_len, D)).astype(f32)
    vc = rng.standard_normal((rows, max_len, D)).astype(f32)
    ang = np.arange(max_len)[:, None] / (10000.0 ** (np.arange(hd // 2)[None, :] * 2.0 / hd))
    cos, sin = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    wo = (rng.standard_normal((D, D)) / np.sqrt(D)).astype(f32)
    qpos = np.full(nq, -1, np.int32)
    for q0, n, s0, _ in runs.tolist():
        if n:
            qpos[q0:q0 + n] = np.arange(s0, s0 + n)
    Q, K, Vc = hip.from_numpy(qkv), hip.from_numpy(kc), hip.from_numpy(vc)
    CS, SN, R = hip.from_numpy(cos), hip.from_numpy(sin), hip.from_numpy(runs)
    rec = ns * H * (4 + hd)
    P = hip.from_numpy(np.full((nq, rec), np.nan, f32))
    W, Y, QP = hip.from_numpy(wo), hip.from_numpy(np.zeros((nq, D), f32)), hip.from_numpy(qpos)
    work = hip.from_numpy(np.zeros(max(4, L.query("pdn_decode_wide_work_floats", nq, D, D)), f32))
    s = hip.stream()
    counters()
    L.call("pdn_kv_append_rows_f32", Q._ptr, 3 * D, CS._ptr, SN._ptr, K._ptr, Vc._ptr, max_len * D, R._ptr, rows, C, nq,
           H, hd, max_len, s)
    L.call("pdn_decode_extend_attention_f32", Q._ptr, 3 * D, CS._ptr, SN._ptr, K._ptr, Vc._ptr, max_len * D, R._ptr, rows,
           C, nq, H, hd, ns, max_len, P._ptr, s)
    first = P.get()
    L.call("pdn_decode_extend_attention_f32", Q._ptr, 3 * D, CS._ptr, SN._ptr, K._ptr, Vc._ptr, max_len * D, R._ptr, rows,
           C, nq, H, hd, ns, max_len, P._ptr, s)
    L.call("pdn_decode_wide_gemm_f32", P._ptr, rec, 3, None, 0.0, ns, hd, W._ptr, D, D, 0, None, Y._ptr, D, 0, None, None,
           QP._ptr, nq, D, D, work._ptr, s)
    assert counters()[33] == 3
    assert np.array_equal(P.get(), first, equal_nan=True)          # two launches: the same bits
    kg, vg, y = K.get(), Vc.get(), Y.get()
    # the caches: the layout's positions hold rotated k / v, each ended prompt's next slot is zero, the rest untouched
    k64, v64 = kc.astype(np.float64), vc.astype(np.float64)
    touched = np.zeros((rows, max_len), bool)
    for r, (q0, n, s0, e) in enumerate(runs.tolist()):
        if not n:
            continue
        p = np.arange(s0, s0 + n)
        k64[r, p] = rotate(qkv[q0:q0 + n, D:2 * D].reshape(n, H, hd).astype(np.float64), cos[p][:, None], sin[p][:, None]).reshape(n, D)
        v64[r, p] = qkv[q0:q0 + n, 2 * D:]
        touched[r, p] = True
        if e and s0 + n < max_len:
            assert not kg[r, s0 + n].any() and not vg[r, s0 + n].any()
            k64[r, s0 + n] = v64[r, s0 + n] = 0
            touched[r, s0 + n] = True
    assert np.array_equal(kg[~touched], kc[~touched]) and np.array_equal(vg[~touched], vc[~touched])
    np.testing.assert_allclose(kg[touched], k64[touched], rtol=1e-5, atol=1e-5)
    assert np.array_equal(vg[touched], v64[touched].astype(f32))
    # attention + merge + Wo against float64
    for r, (q0, n, s0, _) in enumerate(runs.tolist()):
        for j in range(n):
            p = s0 + j
            q = rotate(qkv[q0 + j, :D].reshape(H, hd).astype(np.float64), cos[p][None], sin[p][None])
            sc = np.einsum("hd,thd->ht", q, k64[r, :p + 1].reshape(-1, H, hd)) / np.sqrt(hd)
            e = np.exp(sc - sc.max(-1, keepdims=True))
            o = np.einsum("ht,thd->hd", e / e.sum(-1, keepdims=True), v64[r, :p + 1].reshape(-1, H, hd)).reshape(D)
            np.testing.assert_allclose(y[q0 + j], o @ wo, rtol=2e-4, atol=2e-4, err_msg=f"run {r} query {j}")


_REQ = [(1 + (7 * r) % 23, (5 * r) % 19) for r in range(20)]    # (prompt length, budget): up to 41 positions


@pytest.mark.parametrize("kw", [{}, SAMPLED])
@pytest.mark.parametrize("C", [1, 16, 64])
@pytest.mark.parametrize("S", [1, 8, 16])
def test_serve_chunked_end_to_end(hip, S, C, kw):
    Graph.clear()
    rng = np.random.default_rng(S + C + len(kw))
    prompts = [rng.integers(0, 256, n) for n, _ in _REQ]
    budgets = [b for _, b in _REQ]
    ref, logits = _ragged_reference(prompts, budgets, **kw)
    stops = {int(ref[3, 4]), int(ref[8, 10])}
    m = _model("hip:0", 16)
    for st in ((), stops):
        counters()
        got = _serve_all(m, prompts, budgets, slots=S, stop_ids=st, prefill_chunk=C, **kw)
        c = counters()
        if not st:      # (counters count launches issued from the host: a graph's capture counts, its replays do not)
            assert c[33] > 0 and c[31] > 0, (c[29:], sorted(m._decode_st["graphs"], key=str))
        assert any(len(k) > 2 and k[2] == "mixed" for k in m._decode_st["graphs"]), "no mixed step captured"
        _check(got, ref, logits, prompts, budgets, st, kw)


def test_serve_without_chunk_leaves_counter_33_alone(hip):
    Graph.clear()
    rng = np.random.default_rng(2)
    prompts = [rng.integers(0, 256, 1 + r % 9) for r in range(10)]
    m = _model("hip:0", 16)
    counters()
    _serve_all(m, prompts, 8, slots=4)
    _serve_all(m, prompts, 8, slots=12)
    c = counters()
    assert c[33] == 0 and c[30] > 0
    assert "mixed" not in m._decode_st and all(len(k) == 2 for k in m._decode_st["graphs"])


def test_large_chunk_yields_serve_steps_on_the_gpu(hip):
    """With C past every admission's prompt tokens the steps are serve's: same requests per step, tokens equal or the
    first difference at a margin below 1e-5 (the mixed step's prompt pass rounds differently from serve's)."""
    Graph.clear()
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, 256, 1 + (3 * r) % 11) for r in range(12)]
    budgets = [2 + (5 * r) % 9 for r in range(12)]
    ref, logits = _ragged_reference(prompts, budgets)
    m = _model("hip:0", 16)
    m.eval()
    try:
        with pdn.no_grad():
            a = [(r.copy(), t.copy()) for r, t in m.serve(prompts, budgets, slots=4)]
            b = [(r.copy(), t.copy()) for r, t in m.serve(prompts, budgets, slots=4, prefill_chunk=200)]
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)
    got = [np.array([t for st in b for r_, t in zip(*st) if r_ == r and t >= 0], np.int64) for r in range(12)]
    _check(got, ref, logits, prompts, budgets, set(), {})
    assert [x[0].tolist() for x in a] == [y[0].tolist() for y in b]     # (no stop ids: the steps follow the budgets)
