"""The decode attention of a sliding-window model (csrc/decode_band.hip, include/pdn_banddecode.h) through the C ABI against
a float64 NumPy statement written here: softmax over the keys [lo, pos], lo = max(0, pos - window + 1), the key-range
partials merged.  Partials are NaN-prefilled and every cache row outside [lo, pos] is NaN before the launch, so a key read from
outside the window, an element no workgroup writes, or one it should not write, fails.  Criteria: those of
tests/test_gqa_decode_gpu.py, the same arithmetic (at most 600 keys per range here)."""
import math

import numpy as np
import pytest

from tests.test_gqa_decode_gpu import _rot

pytestmark = pytest.mark.gpu

CASES = [  # B, H, Hkv, hd, n_splits, max_len, window, pos (an int: every row there; a list: the rows form)
    (2, 4, 4, 48, 1, 64, 1, 5),                   # a window of one: only the new key, in LDS; G = 1; register preload
    (1, 6, 2, 48, 4, 64, 16, 7),                  # the window not yet full (lo = 0): plain decode attention, ragged ranges
    (1, 4, 2, 64, 4, 64, 16, 15),                 # the last position before key 0 leaves ...
    (1, 4, 2, 64, 4, 64, 16, 16),                 # ... and the first at which it has
    (1, 8, 2, 64, 4, 64, 2, 40),                  # more ranges than keys: empty-range records
    (2, 8, 1, 32, 1, 700, 600, 650),              # G = 8, generic head dim, two keys per thread, V in the loop
    (1, 4, 2, 128, 2, 400, 300, 399),             # largest head dim, the window ends at the last cache row
    (1, 2, 1, 32, 2, 20000, 64, 19999),           # LDS follows the window, not max_len (pdnj_ refuses this cache)
    (4, 4, 2, 64, 2, 320, 32, [-1, 0, 31, 299]),  # rows form: stopped, unfilled, just-full and slid windows
]


def _run(hip, case):
    from pydynet_amd import _lib
    L = _lib.lib()
    B, H, Hkv, hd, NS, max_len, W, pos = case
    rows = isinstance(pos, list)
    P = np.array(pos if rows else [pos] * B, np.int32)
    G, D, KVD, half = H // Hkv, H * hd, Hkv * hd, hd // 2
    rng = np.random.default_rng(B + H + hd + max_len + W)
    qkv = rng.standard_normal((B, D + 2 * KVD), dtype=np.float32)
    kc, vc = (rng.standard_normal((B, max_len, Hkv, hd), dtype=np.float32) for _ in range(2))
    lo = np.maximum(np.maximum(P, 0) - W + 1, 0)
    for b in range(B):                            # every row outside [lo, p] is NaN (a stopped row: outside [0, 0])
        kc[b, :lo[b]] = vc[b, :lo[b]] = kc[b, max(P[b], 0) + 1:] = vc[b, max(P[b], 0) + 1:] = np.nan
    ang = np.arange(max_len)[:, None] / 10000.0 ** (np.arange(half)[None, :] / half)
    cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    dev = [hip.from_numpy(a) for a in (qkv, cos, sin, kc, vc, P if rows else P[:1])]
    assert L.query("pdnv_decode_attention_supported", H, Hkv, hd, NS, W, max_len) == 1
    runs = []
    for _ in range(2):                            # (the second launch rewrites cache row pos with the same values)
        parts = hip.from_numpy(np.full((B, NS, H, 4 + hd), np.nan, np.float32))
        L.call("pdnv_decode_attention_f32", dev[0]._ptr, D + 2 * KVD, dev[1]._ptr, dev[2]._ptr, dev[3]._ptr, dev[4]._ptr,
               parts._ptr, B, H, Hkv, hd, NS, max_len * KVD, dev[5]._ptr, max_len, W, int(rows), hip.stream())
        runs.append((parts.get(), dev[3].get(), dev[4].get()))
    want, kc_want, vc_want, k_new = np.zeros((B, H, hd)), kc.copy(), vc.copy(), {}
    for b in range(B):
        p = max(int(P[b]), 0)
        c, s = cos[p].astype(np.float64), sin[p].astype(np.float64)
        q = _rot(qkv[b, :D].astype(np.float64).reshape(H, hd), c, s)
        K, V = kc[b, lo[b]:p + 1].astype(np.float64), vc[b, lo[b]:p + 1].astype(np.float64)
        K[-1], V[-1] = _rot(qkv[b, D:D + KVD].astype(np.float64).reshape(Hkv, hd), c, s), qkv[b, D + KVD:].reshape(Hkv, hd)
        if P[b] >= 0:
            k_new[b], vc_want[b, p] = K[-1], qkv[b, D + KVD:].reshape(Hkv, hd)
        sc = np.einsum("hd,thd->ht", q, np.repeat(K, G, axis=1)) / math.sqrt(hd)
        e = np.exp(sc - sc.max(-1, keepdims=True))
        want[b] = np.einsum("ht,thd->hd", e / e.sum(-1, keepdims=True), np.repeat(V, G, axis=1))
    return case, P, lo, runs, want, kc_want, vc_want, k_new


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c[:7]) + f"-{c[7] if isinstance(c[7], int) else 'rows'}")
def test_band_decode_attention(hip, case):
    (B, H, Hkv, hd, NS, max_len, W, _), P, lo, runs, want, kc_want, vc_want, k_new = _run(hip, case)
    parts, kc_got, vc_got = runs[0]
    assert not np.isnan(parts[..., :2]).any() and not np.isnan(parts[..., 4:]).any()
    m, l, o = parts[..., 0].astype(np.float64), parts[..., 1].astype(np.float64), parts[..., 4:].astype(np.float64)
    for b in range(B):                            # ranges without keys: [-inf, 0 | zeros]; the others hold keys
        n = max(int(P[b]), 0) - int(lo[b]) + 1
        for sp in range(NS):
            if sp * -(-n // NS) >= n:
                assert np.all(m[b, sp] == -np.inf) and np.all(l[b, sp] == 0) and np.all(o[b, sp] == 0), (b, sp)
    w = np.exp(m - m.max(1, keepdims=True))
    merged = (w[..., None] * o).sum(1) / (w * l).sum(1)[..., None]
    err = float(np.abs(merged - want).max() / np.abs(want).max())
    assert err < 1e-5, err
    # the caches: row pos = the rotated k and v; every other row -- the NaN rows outside the window too -- untouched
    for b, k in k_new.items():
        p = int(P[b])
        assert np.abs(kc_got[b, p] - k).max() <= 1e-6 * np.abs(k).max(), b
        kc_want[b, p] = kc_got[b, p]
    assert np.array_equal(kc_got, kc_want, equal_nan=True) and np.array_equal(vc_got, vc_want, equal_nan=True)
    assert all(a.tobytes() == b_.tobytes() for a, b_ in zip(runs[0], runs[1]))     # (fixed order: the same bits)


def test_band_decode_supported_range(hip):
    from pydynet_amd import _lib
    L = _lib.lib()
    q = lambda *a: L.query("pdnv_decode_attention_supported", *a)     # H, Hkv, hd, n_splits, window, max_len
    assert [q(16, 1, 48, 1, 8, 64), q(4, 2, 132, 1, 8, 64), q(4, 2, 48, 1, 0, 64), q(4, 2, 48, 65, 8, 64),
            q(4, 2, 48, 1, 8, 64), q(4, 4, 48, 1, 8, 64)] == [0, 0, 0, 0, 1, 1]
    assert q(2, 1, 32, 2, 64, 20000) == 1 and L.query("pdnj_decode_attention_supported", 2, 1, 32, 2, 20000) == 0
