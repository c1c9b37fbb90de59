"""Plain float64 NumPy statements of the four operations behind tests/test_decode_layer_variants.py: the decode attention over
the KV cache with its key-range records (csrc/decode.hip), the attention half of a decode layer (csrc/decode_block.hip), the
feed-forward half (csrc/decode_layer.hip) and the chunked-prefill append / extend attention (csrc/extend.hip).  Nothing here
imports this package or the ABI emulator: every function takes and returns arrays, loops where a loop is the plainest
statement, and leaves strides, tiles and launch shapes to the code under test."""
import numpy as np

F64 = np.float64


def rotate(x, c, s):
    """Interleaved-pair RoPE (llm/llama/model.py:23-44): x (..., hd), c / s (hd / 2,) or broadcastable to (..., hd / 2)."""
    x = np.asarray(x, F64)
    a, b = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2], out[..., 1::2] = a * c - b * s, a * s + b * c
    return out


def key_ranges(T, ns):
    """[t0, t1) of the ns ranges of ceil(T / ns) keys; t0 >= t1: a range without keys."""
    chunk = -(-T // ns) if T > 0 else 0
    return [(sp * chunk, min(T, sp * chunk + chunk)) for sp in range(ns)]


def softmax_record(q, K, V, inv):
    """One head, one key range: q (hd,), K / V (n, hd) -> [m, l, nan, nan | sum_t exp(s_t - m) v_t]; n = 0: [-inf, 0 | zeros]."""
    hd = q.shape[0]
    rec = np.full(4 + hd, np.nan, F64)
    if K.shape[0] == 0:
        rec[0], rec[1], rec[4:] = -np.inf, 0.0, 0.0
        return rec
    s = (K @ q) * inv
    m = s.max()
    e = np.exp(s - m)
    rec[0], rec[1], rec[4:] = m, e.sum(), e @ V
    return rec


def records_of(q, K, V, ranges, limit=None):
    """q (H, hd) rotated, K / V (T, H, hd) -> (len(ranges), H, 4 + hd); `limit`: keys at or past it are masked."""
    H, hd = q.shape
    inv = 1.0 / np.sqrt(F64(hd))
    out = np.empty((len(ranges), H, 4 + hd), F64)
    for sp, (t0, t1) in enumerate(ranges):
        t1 = t1 if limit is None else min(t1, limit)
        t1 = max(t1, t0)
        for h in range(H):
            out[sp, h] = softmax_record(q[h], K[t0:t1, h], V[t0:t1, h], inv)
    return out


def decode_attention(qkv_row, kc_row, vc_row, cos, sin, pos, H, ns):
    """The new token of one sequence at position `pos` (pos < 0: a stopped row, computed at position 0 from its own key
    alone).  qkv_row (3 D,), kc_row / vc_row (max_len, D) of which only rows [0, pos) are read.
    -> records (ns, H, 4 + hd), and the cache row (k rotated (D,), v (D,)) the call appends at `pos` (None when stopped)."""
    D = qkv_row.shape[0] // 3
    hd = D // H
    p = max(int(pos), 0)
    q = rotate(np.asarray(qkv_row[:D], F64).reshape(H, hd), cos[p], sin[p])
    k = rotate(np.asarray(qkv_row[D:2 * D], F64).reshape(H, hd), cos[p], sin[p])
    v = np.asarray(qkv_row[2 * D:3 * D], F64).reshape(H, hd)
    K = np.concatenate([np.asarray(kc_row[:p], F64).reshape(p, H, hd), k[None]])
    V = np.concatenate([np.asarray(vc_row[:p], F64).reshape(p, H, hd), v[None]])
    rec = records_of(q, K, V, key_ranges(p + 1, ns))
    return rec, (None if pos < 0 else (k.reshape(D), v.reshape(D)))


def project(rec, wo):
    """(ns, H, 4 + hd) -> (ns, H, 4 + D): the sums of head h times rows [h hd, (h + 1) hd) of Wo (D, D)."""
    ns, H, w = rec.shape
    hd = w - 4
    wo = np.asarray(wo, F64)
    out = np.full((ns, H, 4 + wo.shape[1]), np.nan, F64)
    out[..., :2] = rec[..., :2]
    for h in range(H):
        out[:, h, 4:] = rec[:, h, 4:] @ wo[h * hd:(h + 1) * hd]
    return out


def merge(rec):
    """(ns, H, 4 + w) records -> (H, w): sum_s exp(m_s - M) o_s / sum_s exp(m_s - M) l_s over the ranges with l > 0."""
    rec = np.asarray(rec, F64)
    ns, H, _ = rec.shape
    out = np.zeros((H, rec.shape[2] - 4), F64)
    for h in range(H):
        live = [s for s in range(ns) if rec[s, h, 1] > 0]
        M = max(rec[s, h, 0] for s in live)
        den = sum(np.exp(rec[s, h, 0] - M) * rec[s, h, 1] for s in live)
        for s in live:
            out[h] += np.exp(rec[s, h, 0] - M) / den * rec[s, h, 4:]
    return out


def rmsnorm(x, w, eps):
    x = np.asarray(x, F64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * np.asarray(w, F64)


def decode_block(base, parts, norm_w, eps, wq, wk, wv, cos, sin, kc_row, vc_row, pos, wo, H, ns):
    """The attention half of a decode layer for one sequence: x = base + sum of parts (n_parts, D); q | k | v of RMSNorm(x);
    RoPE at pos; `ns` ranges of ceil(pos / ns) CACHED keys [0, pos) and one record of the new key alone, each times Wo.
    -> x (D,), records (ns + 1, H, 4 + D), appended cache row (k, v) or None for a stopped row (pos < 0: position 0)."""
    x = np.asarray(base, F64) + (np.asarray(parts, F64).sum(0) if parts is not None and len(parts) else 0.0)
    D = x.shape[0]
    hd = D // H
    n = rmsnorm(x, norm_w, eps)
    p = max(int(pos), 0)
    q = rotate((n @ np.asarray(wq, F64)).reshape(H, hd), cos[p], sin[p])
    k = rotate((n @ np.asarray(wk, F64)).reshape(H, hd), cos[p], sin[p])
    v = (n @ np.asarray(wv, F64)).reshape(H, hd)
    K = np.asarray(kc_row[:p], F64).reshape(p, H, hd)
    V = np.asarray(vc_row[:p], F64).reshape(p, H, hd)
    rec = np.concatenate([records_of(q, K, V, key_ranges(p, ns)), records_of(q, k[None], v[None], [(0, 1)])])
    return x, project(rec, wo), (None if pos < 0 else (k.reshape(D), v.reshape(D)))


def decode_mlp(base, rec, norm_w, eps, wg, wu, wd):
    """One sequence: h = base (+ the merged records (ns, H, 4 + D), summed over heads); n = RMSNorm(h);
    a = silu(n Wg) * (n Wu); parts[j] = a[32 j : 32 j + 32] @ Wd[32 j : 32 j + 32].  -> h (D,), parts (F / 32, D)."""
    h = np.asarray(base, F64)
    if rec is not None:
        h = h + merge(rec).sum(0)
    n = rmsnorm(h, norm_w, eps)
    g, u = n @ np.asarray(wg, F64), n @ np.asarray(wu, F64)
    a = g / (1.0 + np.exp(-g)) * u
    wd = np.asarray(wd, F64)
    return h, np.stack([a[j:j + 32] @ wd[j:j + 32] for j in range(0, a.shape[0], 32)])


def run_taken(q0, n, start, max_run, n_q, max_len):
    return 1 <= n <= max_run and q0 >= 0 and q0 + n <= n_q and start >= 0 and start + n <= max_len


def kv_append(qkv, cos, sin, kc, vc, runs, max_run, H, max_len):
    """qkv (n_q, 3 D); caches (n_runs, max_len, D) float64, written in place: run r = [q0, n, start, ends] stores k of query
    q0 + j rotated by position start + j, and v, at that position of cache row r; `ends` zeroes position start + n when
    there is one."""
    D = qkv.shape[1] // 3
    hd = D // H
    for r, (q0, n, start, ends) in enumerate(runs):
        if not run_taken(q0, n, start, max_run, qkv.shape[0], max_len):
            continue
        for j in range(n):
            p = start + j
            kc[r, p] = rotate(np.asarray(qkv[q0 + j, D:2 * D], F64).reshape(H, hd), cos[p], sin[p]).reshape(D)
            vc[r, p] = qkv[q0 + j, 2 * D:3 * D]
        if ends and start + n < max_len:
            kc[r, start + n] = 0.0
            vc[r, start + n] = 0.0


def extend_attention(qkv, cos, sin, kc, vc, runs, max_run, H, ns, max_len, part):
    """part (n_q, ns, H, 4 + hd) float64, written for the query rows of every taken run: query q0 + j at position start + j
    attends keys [0, start + j] of cache row r, cut into the ns ranges of the run's LAST query (ceil((start + n) / ns))."""
    D = qkv.shape[1] // 3
    hd = D // H
    for r, (q0, n, start, _) in enumerate(runs):
        if not run_taken(q0, n, start, max_run, qkv.shape[0], max_len):
            continue
        T = start + n
        K, V = np.asarray(kc[r, :T], F64).reshape(T, H, hd), np.asarray(vc[r, :T], F64).reshape(T, H, hd)
        for j in range(n):
            p = start + j
            q = rotate(np.asarray(qkv[q0 + j, :D], F64).reshape(H, hd), cos[p], sin[p])
            rec = records_of(q, K, V, key_ranges(T, ns), limit=p + 1)
            rec[..., 2:4] = 0.0
            part[q0 + j] = rec
