"""The penalty entry points (csrc/penalty.hip): the reset and the two apply entries, launch counter 35.  `apply_np` /
`reset_np` are also the references of the GPU tests; both follow pydynet_amd/llm/penalties.py.
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd.llm import penalties
from ._base import view, flat

PENALTY_CHUNK = 1024                                     # vocabulary tokens per workgroup of csrc/penalty.hip


def penalty_chunks(V):
    return -(-V // PENALTY_CHUNK) if V > 0 else 0


def bits_to_rows(words, V):
    """(B, ceil(V / 32)) int32 prompt bits -> (B, V) bool."""
    w = np.asarray(words).view(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(w.shape[0], -1)[:, :V].astype(bool)


def reset_np(counts, seen, start, rows, ids, offsets):
    """pdn_penalty_reset on arrays (in place): counts (B, V), seen (B, W) int32, start (B,)."""
    B, V = counts.shape
    for i, b in enumerate(np.asarray(rows).tolist()):
        if not 0 <= b < B:
            continue
        q = np.asarray(ids[offsets[i]:offsets[i + 1]], np.int64)
        counts[b] = 0
        seen[b] = penalties.seen_bits([q[(q >= 0) & (q < V)]], V)[0]
        start[b] = q.size


def apply_np(z, params, counts=None, seen=None, pos=None, start=None, ids=None, count=False):
    """Either apply entry on arrays: z (B, V) float32 penalised in place (rows with pos < 0 untouched), counts (B, V)
    incremented in place for the fed token when `count`.  Returns the candidates (values (B, n), indices (B, n)) of each
    1024-token chunk: its first maximum (rows skipped: unset, NaN / -1)."""
    B, V = z.shape
    r, p, f = params
    n = penalty_chunks(V)
    cv, ci = np.full((B, n), np.nan, np.float32), np.full((B, n), -1, np.int32)
    for b in range(B):
        pb = 0 if pos is None else int(pos[b])
        if pb < 0:
            continue
        c = np.zeros(V, np.int64) if counts is None else counts[b]
        if count and pb > start[b] and 0 <= ids[b] < V:
            c[int(ids[b])] += 1
        s = np.zeros(V, bool) if seen is None else bits_to_rows(seen[b:b + 1], V)[0]
        z[b] = penalties.penalize(z[b:b + 1], c[None], s[None], r, p, f)[0]
        for j in range(n):
            seg = z[b, j * PENALTY_CHUNK:(j + 1) * PENALTY_CHUNK]
            k = int(np.argmax(seg))
            cv[b, j], ci[b, j] = seg[k], j * PENALTY_CHUNK + k
    return cv, ci


def read_penalty_params(ptr):
    return tuple(float(v) for v in np.array(flat(ptr, 4, np.float32))[:3])


class PenaltyMixin:
    def pdn_penalty_chunks(self, V):
        return penalty_chunks(V)

    def pdn_penalty_reset(self, counts, seen, start, B, V, rows, n_rows, ids, offsets, stream):
        if n_rows == 0:
            return 0
        if not (counts and seen and start and rows and offsets and B > 0 and V > 0 and n_rows > 0):
            return -1
        off = np.array(flat(offsets, n_rows + 1, np.int32))
        reset_np(flat(counts, B * V, np.int32).reshape(B, V), flat(seen, B * -(-V // 32), np.int32).reshape(B, -1),
                 flat(start, B, np.int32), np.array(flat(rows, n_rows, np.int32)),
                 np.array(flat(ids, int(off[-1]), np.int64)) if ids else np.zeros(0, np.int64), off)
        self._count(35)
        return 0

    def _apply(self, logits, rs, B, V, params, counts, seen, pos, pos_rows, cand_v, cand_i, start=None, ids=None, cnt=False):
        Z = view(logits, (B, V), (rs, 1), np.float32)
        C = flat(counts, B * V, np.int32).reshape(B, V) if counts else None
        S = np.array(flat(seen, B * -(-V // 32), np.int32)).reshape(B, -1) if seen else None
        P = None
        if pos:
            P = np.array(flat(pos, B if pos_rows else 1, np.int32))
            P = P if pos_rows else np.full(B, P[0])
        st = np.array(flat(start, B, np.int32)) if start else None
        fed = np.array(flat(ids, B, np.int64)) if ids else None
        z = np.array(Z)
        c64 = None if C is None else C.astype(np.int64)
        cv, ci = apply_np(z, read_penalty_params(params), c64, S, P, st, fed, cnt)
        Z[...] = z
        if C is not None and cnt:
            C[...] = c64
        if cand_v:
            n = penalty_chunks(V)
            V_, I_ = flat(cand_v, B * n, np.float32).reshape(B, n), flat(cand_i, B * n, np.int32).reshape(B, n)
            live = ~np.isnan(cv[:, 0]) if n else np.zeros(B, bool)
            V_[live], I_[live] = cv[live], ci[live]
        self._count(35)
        return 0

    def pdn_penalty_step_f32(self, logits, rs, B, V, params, counts, seen, start, ids, pos, pos_per_row, cand_v, cand_i,
                             stream):
        if B == 0:
            return 0
        if not (logits and params and counts and seen and start and ids and pos and V > 0 and rs >= V):
            return -1
        return self._apply(logits, rs, B, V, params, counts, seen, pos, pos_per_row, cand_v, cand_i, start, ids, True)

    def pdn_penalty_rows_f32(self, logits, rs, B, V, params, counts, seen, pos, cand_v, cand_i, stream):
        if B == 0:
            return 0
        if not (logits and params and V > 0 and rs >= V):
            return -1
        return self._apply(logits, rs, B, V, params, counts, seen, pos, 1, cand_v, cand_i)
