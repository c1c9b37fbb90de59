"""The beam-search entry points (csrc/beam.hip): the top-k, select and KV-cache reorder launches, launch counter 32.  They
run the statement of pydynet_amd/llm/beam.py, so the emulated fast path and the `cpu` device compute the same bits.
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd.llm import beam
from ._base import view, flat


class BeamMixin:
    def pdn_beam_topk_rows_f32(self, logits, rs, B, V, W, first, pos, stops, S, cand_lp, cand_id, stop_lp, stream):
        if B == 0:
            return 0
        if not (logits and cand_lp and cand_id and 1 <= W <= 16 and 0 <= S <= 16 and V - S >= W and rs >= V
                and (S == 0 or (stops and stop_lp)) and (not first or B % W == 0)):
            return -1
        P = np.array(flat(pos, B, np.int32)) if pos else np.zeros(B, np.int32)
        st = np.array(flat(stops, S, np.int32), np.int64) if S else np.zeros(0, np.int64)
        rows = [r for r in range(B) if P[r] >= 0 and (not first or r % W == 0)]
        if rows:
            src = [r // W if first else r for r in rows]
            z = np.array(view(logits, (max(src) + 1, V), (rs, 1), np.float32))[src]
            lp, ids, slp = beam.topk_rows(z, W, st)
            flat(cand_lp, B * W).reshape(B, W)[rows] = lp
            flat(cand_id, B * W, np.int32).reshape(B, W)[rows] = ids
            if S:
                flat(stop_lp, B * S).reshape(B, S)[rows] = slp
        self._count(32)
        return 0

    def pdn_beam_select_f32(self, cand_lp, cand_id, stop_lp, stops, S, G, W, first, scores, next_ids, parent, pos, step,
                            arrive, live_acc, hist, n_hist, fin_n, fin, live_out, n_live, emb, emb_rs, D, x_next, stream):
        if G == 0:
            return 0
        if not (cand_lp and cand_id and scores and next_ids and parent and pos and step and arrive and live_acc and fin_n
                and fin and 1 <= W <= 16 and 0 <= S <= 16 and (S == 0 or (stops and stop_lp))):
            return -1
        B = G * W
        cl = np.array(flat(cand_lp, B * W).reshape(B, W))
        ci = np.array(flat(cand_id, B * W, np.int32).reshape(B, W), np.int64)
        sl = np.array(flat(stop_lp, B * S).reshape(B, S)) if S else np.zeros((B, 0), np.float32)
        st = np.array(flat(stops, S, np.int32), np.int64) if S else np.zeros(0, np.int64)
        sc, P, par = flat(scores, B), flat(pos, B, np.int32), flat(parent, B, np.int32)
        ids = flat(next_ids, B, np.int64)
        s = int(flat(step, 1, np.int32)[0])
        H = flat(hist, n_hist * B * 2, np.int32).reshape(n_hist, B, 2) if hist else None
        Fn, F = flat(fin_n, G, np.int32), flat(fin, G * (2 * W - 1) * 4, np.int32).reshape(G, 2 * W - 1, 4)
        live = 0
        for g in range(G):
            r0 = g * W
            p0 = int(P[r0])
            if p0 < 0:
                continue
            nb = 1 if first else W
            tok, pb, nsc, fins = beam.select_group(sc[r0:r0 + W], cl[r0:r0 + nb], ci[r0:r0 + nb], sl[r0:r0 + nb], st, W,
                                                   bool(first))
            n = int(Fn[g])
            for (b, t, raw) in fins:
                F[g, n] = (s, b, t, np.float32(raw).view(np.int32))
                n += 1
            Fn[g] = n
            done = n >= W
            if H is not None and s < n_hist:
                H[s, r0:r0 + W, 0], H[s, r0:r0 + W, 1] = tok, pb
            sc[r0:r0 + W], ids[r0:r0 + W] = nsc, tok
            par[r0:r0 + W] = np.arange(r0, r0 + W) if done else r0 + pb
            P[r0:r0 + W] = -1 if done else p0 + 1
            if x_next and not done:
                X = flat(x_next, B * D).reshape(B, D)
                for j in range(W):
                    X[r0 + j] = flat(emb + 4 * int(tok[j]) * emb_rs, D)
            live += not done
        if live_out and s < n_live:
            flat(live_out + 8 * s, 1, np.int64)[0] = live
        flat(step, 1, np.int32)[0] = s + 1
        self._count(32)
        return 0

    def pdn_kv_reorder_rows_f32(self, caches, n_tensors, bs, B, max_len, D, parent, pos, stream):
        if n_tensors == 0 or B == 0:
            return 0
        if not (caches and parent and pos and 0 < B <= 256 and D % 4 == 0 and bs >= max_len * D):
            return -1
        par, P = np.array(flat(parent, B, np.int32)), np.array(flat(pos, B, np.int32))
        for c in flat(caches, n_tensors, np.int64):
            rows = view(int(c), (B, max_len * D), (bs, 1), np.float32)
            old = np.array(rows)                          # (the gather reads the rows as they were before the launch)
            for r in range(B):
                n = min(int(P[r]), max_len)
                if par[r] != r and 0 <= par[r] < B and n > 0:
                    rows[r, :n * D] = old[par[r], :n * D]
        self._count(32)
        return 0
