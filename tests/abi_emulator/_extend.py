"""The entry points that extend several positions of a row in one step: chunked prefill (csrc/extend.hip: the KV append and
the multi-query extend attention of the mixed step; launch counter 33), speculative decoding (csrc/speculative.hip: the
draft kernel and the two verify ticks; counter 34) and the prefix cache's row-to-row copy (csrc/prefix.hip; counter 38).
`append_np` / `extend_np`, `draft_np` / `settle_np` and `copy_prefix_np` are also the references of the GPU tests; the
speculative ones follow pydynet_amd/llm/speculative.py.
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd.llm import sampling, speculative
from ._base import view, flat
from ._decode_rows import _greedy_pick
from ._sampling import read_sample_params


# -- chunked prefill --------------------------------------------------------------------------------------------------
def rotate(x, c, s):
    """Interleaved-pair RoPE of rows x (..., hd) with cos / sin rows (..., hd / 2)."""
    a, b = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2], out[..., 1::2] = a * c - b * s, a * s + b * c
    return out


def run_ok(q0, n, s0, max_run, n_q, max_len):
    return 0 < n <= max_run and q0 >= 0 and q0 + n <= n_q and s0 >= 0 and s0 + n <= max_len


def append_np(qkv, cos, sin, kc, vc, runs, max_run, H, hd, max_len):
    """pdn_kv_append_rows_f32 on arrays: qkv (n_q, >= 3 D), caches (rows, max_len, D) written in place."""
    D = H * hd
    for r, (q0, n, s0, ends) in enumerate(np.asarray(runs).reshape(-1, 4).tolist()):
        if not run_ok(q0, n, s0, max_run, qkv.shape[0], max_len):
            continue
        p = np.arange(s0, s0 + n)
        k = qkv[q0:q0 + n, D:2 * D].reshape(n, H, hd)
        kc[r, s0:s0 + n] = rotate(k, cos[p][:, None, :], sin[p][:, None, :]).reshape(n, D)
        vc[r, s0:s0 + n] = qkv[q0:q0 + n, 2 * D:3 * D]
        if ends and s0 + n < max_len:
            kc[r, s0 + n] = 0
            vc[r, s0 + n] = 0


def extend_np(qkv, cos, sin, kc, vc, runs, max_run, H, hd, ns, max_len, part):
    """pdn_decode_extend_attention_f32 on arrays: part (n_q, ns, H, 4 + hd) written for the query rows of every run."""
    D = H * hd
    inv = 1.0 / np.sqrt(np.asarray(hd, qkv.dtype))
    for r, (q0, n, s0, _) in enumerate(np.asarray(runs).reshape(-1, 4).tolist()):
        if not run_ok(q0, n, s0, max_run, qkv.shape[0], max_len):
            continue
        T = s0 + n
        chunk = -(-T // ns)
        for j in range(n):
            p = s0 + j
            q = rotate(qkv[q0 + j, :D].reshape(H, hd), cos[p][None, :], sin[p][None, :])
            for sp in range(ns):
                t0, t1 = sp * chunk, min(T, sp * chunk + chunk, p + 1)
                rec = part[q0 + j, sp]
                rec[...] = 0
                if t1 <= t0:
                    rec[:, 0] = -np.inf
                    continue
                k = kc[r, t0:t1].reshape(-1, H, hd)
                v = vc[r, t0:t1].reshape(-1, H, hd)
                s = np.einsum("hd,thd->ht", q, k) * inv
                m = s.max(-1)
                e = np.exp(s - m[:, None])
                rec[:, 0], rec[:, 1] = m, e.sum(-1)
                rec[:, 4:] = np.einsum("ht,thd->hd", e, v)


# -- speculative decoding ---------------------------------------------------------------------------------------------
def draft_np(hist, hlen, pos, left, k):
    """pdn_spec_draft_rows on arrays: (tokens (B (k + 1),) int64, qpos (B (k + 1),) int32, runs (B, 4) int32)."""
    B, K1 = len(pos), k + 1
    tok, qpos, runs = np.zeros(B * K1, np.int64), np.full(B * K1, -1, np.int32), np.zeros((B, 4), np.int32)
    for b in range(B):
        runs[b, 0] = b * K1
        if pos[b] < 0 or hlen[b] < 1:
            continue
        h = np.asarray(hist[b][:hlen[b]], np.int64)
        d = speculative.draft(h, k, left[b])
        tok[b * K1] = h[-1]
        tok[b * K1 + 1:b * K1 + 1 + d.size] = d
        qpos[b * K1:b * K1 + 1 + d.size] = pos[b] + np.arange(d.size + 1)
        runs[b] = (b * K1, d.size + 1, pos[b], 0)
    return tok, qpos, runs


def settle_np(tok, qpos, picks, k, hist, hlen, pos, left, stops):
    """The accept part of both ticks on arrays (hist / hlen / pos / left updated in place): the (B, k + 4) mailbox slot."""
    B, K1 = len(pos), k + 1
    out = np.full((B, k + 4), -1, np.int64)
    out[:, :3] = 0
    for b in range(B):
        if pos[b] < 0:
            continue
        d = 0
        while d < k and qpos[b * K1 + d + 1] >= 0:
            d += 1
        fed, got = tok[b * K1:b * K1 + d + 1], picks[b * K1:b * K1 + d + 1]
        y, a, hit = speculative.accept(fed, got, left[b], stops)
        c = y.size
        hist[b][hlen[b]:hlen[b] + c] = y
        hlen[b] += c
        left[b] -= c
        pos[b] = -1 if (hit or left[b] <= 0) else pos[b] + c
        out[b, :3] = (c, d, min(a, c))
        out[b, 3:3 + c] = y
    return out


def _stops(mask_ptr, V):
    if not mask_ptr:
        return np.zeros(0, np.int64)
    m = np.array(flat(mask_ptr, -(-V // 32), np.int32)).view(np.uint32)
    bits = (m[:, None] >> np.arange(32, dtype=np.uint32)) & 1
    return np.flatnonzero(bits.reshape(-1))


# -- prefix cache -----------------------------------------------------------------------------------------------------
MAX_COPIES = 256


def copy_prefix_np(caches, dst, src, lens):
    """pdn_kv_copy_prefix_rows_f32 on arrays: each cache (n_rows, max_len, D), written in place.  Snapshot, then copy:
    every source is read as it was before the call."""
    for c in caches:
        n_rows, max_len = c.shape[:2]
        before = np.array(c)
        for d, s, n in zip(np.asarray(dst).tolist(), np.asarray(src).tolist(), np.asarray(lens).tolist()):
            if d == s or n <= 0 or not (0 <= d < n_rows and 0 <= s < n_rows):
                continue
            n = min(n, max_len)
            c[d, :n] = before[s, :n]


class ExtendMixin:
    def pdn_decode_mixed_supported(self, D, H, hd, F, V, max_len):
        return int(H > 0 and hd > 0 and hd * H == D and hd % 4 == 0 and hd <= 256 and F > 0 and F % 4 == 0
                   and 0 < V <= 1 << 23 and 0 < max_len and max_len * 4 <= 60 * 1024)

    @staticmethod
    def _arrays(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, n_q, H, hd, max_len):
        D = H * hd
        return (np.array(view(qkv, (n_q, 3 * D), (rs, 1), np.float32)),
                np.array(flat(cos, max_len * hd // 2)).reshape(max_len, hd // 2),
                np.array(flat(sin, max_len * hd // 2)).reshape(max_len, hd // 2),
                view(kc, (n_runs, max_len, D), (cbs, D, 1), np.float32),
                view(vc, (n_runs, max_len, D), (cbs, D, 1), np.float32),
                np.array(flat(runs, 4 * n_runs, np.int32)).reshape(n_runs, 4))

    def pdn_kv_append_rows_f32(self, qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, max_run, n_q, H, hd, max_len, stream):
        if n_runs == 0:
            return 0
        if not (qkv and kc and vc and runs and max_run > 0 and n_q > 0 and hd % 4 == 0 and cbs >= max_len * H * hd):
            return -1
        Q, c, s, K, Vc, R = self._arrays(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, n_q, H, hd, max_len)
        append_np(Q, c, s, K, Vc, R, max_run, H, hd, max_len)
        self._count(33)
        return 0

    def pdn_decode_extend_attention_f32(self, qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, max_run, n_q, H, hd, ns, max_len,
                                        part, stream):
        if n_runs == 0:
            return 0
        if not (qkv and kc and vc and runs and part and max_run > 0 and n_q > 0 and hd % 4 == 0 and 1 <= ns <= 64):
            return -1
        Q, c, s, K, Vc, R = self._arrays(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, n_q, H, hd, max_len)
        P = flat(part, n_q * ns * H * (4 + hd)).reshape(n_q, ns, H, 4 + hd)
        extend_np(Q, c, s, np.array(K), np.array(Vc), R, max_run, H, hd, ns, max_len, P)
        self._count(33)
        return 0

    def pdn_spec_draft_rows(self, hist, hs, hlen, pos, left, B, k, tokens, qpos, runs, stream):
        if not (hist and hlen and pos and left and tokens and qpos and runs and B > 0 and 0 <= k <= 16 and hs > 0):
            return -1
        H = flat(hist, B * hs, np.int32).reshape(B, hs)
        t, q, r = draft_np(H, np.array(flat(hlen, B, np.int32)), np.array(flat(pos, B, np.int32)),
                           np.array(flat(left, B, np.int32)), k)
        flat(tokens, B * (k + 1), np.int64)[...] = t
        flat(qpos, B * (k + 1), np.int32)[...] = q
        flat(runs, 4 * B, np.int32)[...] = r.reshape(-1)
        self._count(34)
        return 0

    def _spec_tick(self, picks_of, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step, mailbox, V):
        R = B * (k + 1)
        q = np.array(flat(qpos, R, np.int32))
        P = flat(picks, R, np.int64)
        for r in np.flatnonzero(q >= 0):
            P[r] = picks_of(int(r), int(q[r]))
        H, HL, PS, LF = (flat(hist, B * hs, np.int32).reshape(B, hs), flat(hlen, B, np.int32), flat(pos, B, np.int32),
                         flat(left, B, np.int32))
        hl, ps, lf = (np.array(a, np.int64) for a in (HL, PS, LF))
        V = int(V or np.array(P)[q >= 0].max(initial=0) + 1)        # (the pick tick: bits up to the largest pick)
        out = settle_np(np.array(flat(tokens, R, np.int64)), q, np.array(P), k, H, hl, ps, lf, _stops(stop, V))
        HL[...], PS[...], LF[...] = hl, ps, lf
        s = flat(step, 1, np.int32)
        mb = int(flat(mailbox, 1, np.int64)[0]) if mailbox else 0
        if mb:
            flat(mb + 8 * int(s[0]) * B * (k + 4), B * (k + 4), np.int64)[...] = out.reshape(-1)
        s[0] += 1
        self._count(34)
        return 0

    def pdn_spec_verify_pick_tick_f32(self, vals, args, n, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step,
                                      mailbox, stream):
        if not (vals and args and n > 0 and tokens and qpos and picks and hist and step and B > 0 and 0 <= k <= 16):
            return -1
        return self._spec_tick(_greedy_pick(vals, args, B * (k + 1), n), tokens, qpos, B, k, picks, hist, hs, hlen, pos,
                               left, stop, step, mailbox, 0)

    def pdn_spec_verify_sample_tick_f32(self, logits, rs, V, params, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left,
                                        stop, step, mailbox, stream):
        if not (logits and params and V > 0 and rs >= V and tokens and qpos and picks and hist and step and B > 0):
            return -1
        T, tk, tp, seed = read_sample_params(params)
        Z = flat(logits, B * (k + 1) * rs, np.float32).reshape(-1, rs)[:, :V]

        def draw(r, p):
            return int(sampling.sample_rows_np(np.array(Z[r:r + 1]), p, T, tk, tp, seed, rows=[r // (k + 1)])[0])
        return self._spec_tick(draw, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step, mailbox, V)

    def pdn_kv_copy_prefix_rows_f32(self, caches, n_tensors, bs, n_rows, max_len, D, dst, src, lens, n_copies, stream):
        if n_tensors == 0 or n_copies == 0:
            return 0
        if not (caches and dst and src and lens and n_tensors > 0 and n_rows > 0 and 0 < n_copies <= MAX_COPIES
                and max_len > 0 and D > 0 and bs >= max_len * D):
            return -1
        ptrs = np.array(flat(caches, n_tensors, np.int64))
        copy_prefix_np([view(int(p), (n_rows, max_len, D), (bs, D, 1), np.float32) for p in ptrs],
                       *(np.array(flat(a, n_copies, np.int32)) for a in (dst, src, lens)))
        self._count(38)
        return 0
