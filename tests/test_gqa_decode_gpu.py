"""The decode attention of a grouped-query model (csrc/decode_gqa.hip, include/pdn_gqdecode.h) through the C ABI against a
float64 NumPy statement written here: K / V repeated along the head axis, softmax over the keys [0, pos], the key-range
partials merged.  Partials are NaN-prefilled and the caches hold random sentinels, so an element no workgroup writes, or one
it should not write, fails.  Tolerance: the criterion of tests/test_decode_layer_variants.py for
pdn_decode_attention_rows_f32 (the same arithmetic, at most 300 keys per range here): max |got - ref| / max |ref| < 1e-5 for
the merged row.  The appended key is two fp32 products and a sum per element: held to 1e-6 of the largest; the value and
every other cache element to equality."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [  # B, H, Hkv, hd, n_splits, max_len, pos (an int: every row there; a list: the rows form)
    (2, 4, 2, 48, 1, 64, 0),                      # only the new key, which lives in LDS alone; the register-preload path
    (1, 6, 2, 48, 4, 600, 299),                   # G = 3, ragged ranges of 75 keys, the owner in the last range
    (1, 8, 2, 64, 4, 64, 2),                      # ranges without keys: -inf / 0 / zero records
    (2, 8, 1, 32, 1, 400, 300),                   # multi-query (G = 8), generic-hd path: two keys per thread, V in the loop
    (1, 4, 2, 128, 2, 300, 257),                  # largest head dim
    (4, 4, 2, 64, 2, 320, [-1, 0, 5, 299]),       # a position per row, one stopped
]


def _rot(x, c, s):
    out = np.empty_like(x)
    out[..., 0::2], out[..., 1::2] = x[..., 0::2] * c - x[..., 1::2] * s, x[..., 0::2] * s + x[..., 1::2] * c
    return out


def _run(hip, case):
    from pydynet_amd import _lib
    L = _lib.lib()
    B, H, Hkv, hd, NS, max_len, pos = case
    rows = isinstance(pos, list)
    P = np.array(pos if rows else [pos] * B, np.int32)
    G, D, KVD, half = H // Hkv, H * hd, Hkv * hd, hd // 2
    rng = np.random.default_rng(B + H + hd + max_len)
    qkv = rng.standard_normal((B, D + 2 * KVD), dtype=np.float32)
    kc, vc = (rng.standard_normal((B, max_len, Hkv, hd), dtype=np.float32) for _ in range(2))
    ang = np.arange(max_len)[:, None] / 10000.0 ** (np.arange(half)[None, :] / half)
    cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    dev = [hip.from_numpy(a) for a in (qkv, cos, sin, kc, vc, P if rows else P[:1])]
    assert L.query("pdnj_decode_attention_supported", H, Hkv, hd, NS, max_len) == 1
    runs = []
    for _ in range(2):                            # (the second launch rewrites cache row pos with the same values)
        parts = hip.from_numpy(np.full((B, NS, H, 4 + hd), np.nan, np.float32))
        L.call("pdnj_decode_attention_f32", dev[0]._ptr, D + 2 * KVD, dev[1]._ptr, dev[2]._ptr, dev[3]._ptr, dev[4]._ptr,
               parts._ptr, B, H, Hkv, hd, NS, max_len * KVD, dev[5]._ptr, max_len, int(rows), hip.stream())
        runs.append((parts.get(), dev[3].get(), dev[4].get()))
    # the statement, float64
    want, kc_want, vc_want, k_new = np.zeros((B, H, hd)), kc.copy(), vc.copy(), {}
    for b in range(B):
        p = max(int(P[b]), 0)
        c, s = cos[p].astype(np.float64), sin[p].astype(np.float64)
        q = _rot(qkv[b, :D].astype(np.float64).reshape(H, hd), c, s)
        K, V = kc[b, :p + 1].astype(np.float64), vc[b, :p + 1].astype(np.float64)
        K[p], V[p] = _rot(qkv[b, D:D + KVD].astype(np.float64).reshape(Hkv, hd), c, s), qkv[b, D + KVD:].reshape(Hkv, hd)
        if P[b] >= 0:
            k_new[b], vc_want[b, p] = K[p], qkv[b, D + KVD:].reshape(Hkv, hd)
        sc = np.einsum("hd,thd->ht", q, np.repeat(K, G, axis=1)) / math.sqrt(hd)
        e = np.exp(sc - sc.max(-1, keepdims=True))
        want[b] = np.einsum("ht,thd->hd", e / e.sum(-1, keepdims=True), np.repeat(V, G, axis=1))
    return case, P, runs, want, kc_want, vc_want, k_new


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:6]))
def test_gqa_decode_attention(hip, case):
    (B, H, Hkv, hd, NS, max_len, _), P, runs, want, kc_want, vc_want, k_new = _run(hip, case)
    parts, kc_got, vc_got = runs[0]
    assert not np.isnan(parts[..., :2]).any() and not np.isnan(parts[..., 4:]).any()
    m, l, o = parts[..., 0].astype(np.float64), parts[..., 1].astype(np.float64), parts[..., 4:].astype(np.float64)
    for b in range(B):                            # ranges without keys: [-inf, 0 | zeros]
        T = max(int(P[b]), 0) + 1
        for sp in range(NS):
            if sp * -(-T // NS) >= T:
                assert np.all(m[b, sp] == -np.inf) and np.all(l[b, sp] == 0) and np.all(o[b, sp] == 0), (b, sp)
    w = np.exp(m - m.max(1, keepdims=True))
    merged = (w[..., None] * o).sum(1) / (w * l).sum(1)[..., None]
    err = float(np.abs(merged - want).max() / np.abs(want).max())
    print(f"merged against float64: {err:.2e}")
    assert err < 1e-5, err
    # the caches: row pos = the rotated k and v, everything else -- a stopped row's whole cache -- untouched
    for b, k in k_new.items():
        p = int(P[b])
        assert np.abs(kc_got[b, p] - k).max() <= 1e-6 * np.abs(k).max(), b
        kc_want[b, p] = kc_got[b, p]
    assert np.array_equal(kc_got, kc_want) and np.array_equal(vc_got, vc_want)
    # no atomics, a fixed order: a second launch gives the same bits
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(runs[0], runs[1]))


def test_gqa_decode_supported_range(hip):
    from pydynet_amd import _lib
    L = _lib.lib()
    assert [L.query("pdnj_decode_attention_supported", H, Hkv, hd, 1, 64) for H, Hkv, hd in
            ((4, 4, 48), (16, 1, 48), (4, 2, 132), (4, 2, 48))] == [0, 0, 0, 1]
