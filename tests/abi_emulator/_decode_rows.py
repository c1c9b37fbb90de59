"""The decode step with a position per row: the ragged `*_rows_f32` entries (csrc/decode.hip, decode_block.hip, sample.hip,
attention.hip; launch counter 29), the continuous-batching `*_slots_f32` ticks and pdn_kv_store_slots_f32 (csrc/serve.hip;
counter 30), and the wide step for 9 to 256 rows (csrc/decode_wide.hip: the MFMA product with its load modes and epilogues,
the workgroup-per-row ticks; counter 31).  Each per-row entry runs the scalar statement of _decode.py once per row, at that
row's position (a stopped row, pos < 0: at position 0, its cache slot put back afterwards).  The sample ticks count in 28 as
well and the wide ticks in 29 / 30, as the real ones do.
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd.llm import sampling
from ._base import view, flat
from ._sampling import read_sample_params

TN = 32                                   # columns per candidate block (csrc/decode_wide.hip: WD_TN)


def gemm_np(X, mode, norm_w, eps, ns, hd, W, bias, K):
    """The product of pdn_decode_wide_gemm_f32 before its epilogue: A(X) @ W + bias, float32 (X: the input rows as
    the entry reads them; W: (K, N) float32)."""
    B = X.shape[0]
    if mode == 3:
        H = K // hd
        R = X[:, :ns * H * (4 + hd)].reshape(B, ns, H, 4 + hd)
        m, l, o = R[..., 0], R[..., 1], R[..., 4:]
        m = np.where(l > 0, m, -np.inf)
        w = np.where(l > 0, np.exp(m - m.max(1, keepdims=True)), 0).astype(np.float32)
        a = ((w[..., None] * o).sum(1) / (w * l).sum(1)[..., None]).reshape(B, K)
    elif mode == 2:
        g, u = X[:, :K], X[:, K:2 * K]
        a = g / (np.float32(1) + np.exp(-g)) * u
    elif mode == 1:
        a = X[:, :K] / np.sqrt((X[:, :K] * X[:, :K]).mean(-1, keepdims=True) + np.float32(eps)) * norm_w
    else:
        a = X[:, :K]
    out = (a.astype(np.float32) @ W).astype(np.float32)
    return out + bias if bias is not None else out


def candidates(out):
    """First maximum and its column per row and 32-column block (the epi 2 candidates)."""
    B, N = out.shape
    nb = -(-N // TN)
    v, a = np.empty((B, nb), np.float32), np.empty((B, nb), np.int32)
    for j in range(nb):
        seg = out[:, j * TN:(j + 1) * TN]
        v[:, j], a[:, j] = seg.max(-1), j * TN + seg.argmax(-1)
    return v, a


def _off(ptr, floats):
    return ptr + 4 * floats if ptr else ptr


def _greedy_pick(vals, args, B, n):
    """pick(b, position) -> the smallest index among row b's largest candidates."""
    v = np.array(flat(vals, B * n).reshape(B, n))
    a = np.array(flat(args, B * n, np.int32).reshape(B, n))
    return lambda b, p: a[b][v[b] == v[b].max()].min()


def _sampled_pick(logits, rs, B, V, params, rows):
    """pick(b, position) -> row b's draw, on the random stream of request rows[b]."""
    T, k, p_, seed = read_sample_params(params)
    z = np.array(view(logits, (B, V), (rs, 1), np.float32))
    return lambda b, p: (sampling.sample_rows_np(z[b:b + 1], p, T, k, p_, seed, rows=[int(rows[b])])[0] if T > 0
                         else z[b].argmax())


class DecodeRowsMixin:
    # -- the layer launches, once per row -----------------------------------------------------------------------------
    def _per_row(self, B, pos, kc, vc, cbs, D, run):
        """run(b, pos_ptr) for every row with a one-element position buffer; a stopped row's slot 0 is put back."""
        p = np.array(flat(pos, B, np.int32))
        for b in range(B):
            one = np.array([max(int(p[b]), 0)], np.int32)
            kslot, vslot = kc + 4 * b * cbs, vc + 4 * b * cbs
            keep = (np.array(flat(kslot, D)), np.array(flat(vslot, D))) if p[b] < 0 else None
            rc = run(b, one.ctypes.data)
            if keep is not None:
                flat(kslot, D)[...], flat(vslot, D)[...] = keep
            if rc:
                return rc
        self._count(29)
        return 0

    def pdn_decode_block_rows_f32(self, base, base_rs, parts, n_parts, parts_rs, x_out, x_out_rs, norm_w, eps, Wqkv, w_rs,
                                  w_bs, cos, sin, kc, vc, cbs, pos, max_len, Wo, wo_rs, recs, B, H, hd, NS, stream):
        D = H * hd
        if B > 8:
            return -1
        rr = (NS + 1) * H * (4 + D)
        return self._per_row(B, pos, kc, vc, cbs, D, lambda b, p: self.pdn_decode_block_f32(
            _off(base, b * base_rs), base_rs, _off(parts, b * parts_rs), n_parts, parts_rs, _off(x_out, b * x_out_rs),
            x_out_rs, norm_w, eps, Wqkv, w_rs, w_bs, cos, sin, _off(kc, b * cbs), _off(vc, b * cbs), cbs, p, max_len, Wo,
            wo_rs, _off(recs, b * rr), 1, H, hd, NS, stream))

    def pdn_decode_attention_rows_f32(self, qkv, rs, cos, sin, kc, vc, parts, B, H, hd, NS, cbs, pos, max_len, stream):
        rr = NS * H * (4 + hd)
        return self._per_row(B, pos, kc, vc, cbs, H * hd, lambda b, p: self.pdn_decode_attention_f32(
            _off(qkv, b * rs), rs, cos, sin, _off(kc, b * cbs), _off(vc, b * cbs), _off(parts, b * rr), 1, H, hd, NS, cbs,
            p, max_len, stream))

    def pdn_decode_attention_oproj_rows_f32(self, qkv, rs, cos, sin, kc, vc, Wo, wo_rs, recs, B, H, hd, NS, cbs, pos,
                                            max_len, stream):
        D = H * hd
        rr = NS * H * (4 + D)
        return self._per_row(B, pos, kc, vc, cbs, D, lambda b, p: self.pdn_decode_attention_oproj_f32(
            _off(qkv, b * rs), rs, cos, sin, _off(kc, b * cbs), _off(vc, b * cbs), Wo, wo_rs, _off(recs, b * rr), 1, H, hd,
            NS, cbs, p, max_len, stream))

    def pdn_attention_decode_rows_f32(self, q, kc, vc, o, B, H, lens, max_T, hd, cbs, stream):
        D = H * hd
        T = np.clip(np.array(flat(lens, B, np.int32)), 1, max_T)
        for b in range(B):
            self.pdn_attention_decode_f32(_off(q, b * D), _off(kc, b * cbs), _off(vc, b * cbs), _off(o, b * D), 1, H,
                                          int(T[b]), hd, cbs, stream)
        self._count(29)
        return 0

    # -- the per-row tick: the rows form (counter 29) and, with `left` and `ring`, the slots form (counter 30) ----------
    def _tick(self, pick, B, ids, pos, step, stop, hist, emb, emb_rs, D, x_next, left=None, ring=0):
        """The tick around pick(b, position) -> token.  The slots form adds a budget per row (`left`: a row stops when it
        reaches 0) and writes its history into a ring of `ring` steps."""
        P, Lf = flat(pos, B, np.int32), flat(left, B, np.int32) if left else None
        s = int(flat(step, 1, np.int32)[0])
        hrow = flat(int(flat(hist, 1, np.int64)[0]) + 8 * (s % ring if ring else s) * B, B, np.int64) if hist else None
        for b in range(B):
            p = int(P[b])
            if p < 0:
                if hrow is not None:
                    hrow[b] = -1
                continue
            tok = int(pick(b, p))
            flat(ids, B, np.int64)[b] = tok
            if hrow is not None:
                hrow[b] = tok
            if emb:
                flat(x_next, B * D).reshape(B, D)[b] = flat(emb + 4 * tok * emb_rs, D)
            hit = False
            if stop:
                mask = np.array(flat(stop, tok // 32 + 1, np.int32)).view(np.uint32)
                hit = bool((mask[tok >> 5] >> np.uint32(tok & 31)) & 1)
            if Lf is not None:
                Lf[b] -= 1
                hit = hit or Lf[b] <= 0
            P[b] = -1 if hit else p + 1
        flat(step, 1, np.int32)[0] = s + 1
        self._count(29 if Lf is None else 30)
        return 0

    def _sample_tick(self, logits, rs, B, V, params, rows, *tick, **slots):
        rc = self._tick(_sampled_pick(logits, rs, B, V, params, rows), B, *tick, **slots)
        scratch = np.zeros(1, np.int64)                  # (counter 28 as well, as the real tick: one launch of the sampler)
        self.pdn_sample_rows_f32(logits, rs, 1, V, params, 0, scratch.ctypes.data, None)
        return rc

    def pdn_decode_pick_tick_rows_f32(self, vals, args, B, n, ids, pos, step, stop, hist, emb, emb_rs, D, x_next, stream):
        return self._tick(_greedy_pick(vals, args, B, n), B, ids, pos, step, stop, hist, emb, emb_rs, D, x_next)

    def pdn_decode_sample_tick_rows_f32(self, logits, rs, B, V, params, ids, pos, step, stop, hist, emb, emb_rs, D, x_next,
                                        stream):
        return self._sample_tick(logits, rs, B, V, params, range(B), ids, pos, step, stop, hist, emb, emb_rs, D, x_next)

    def pdn_decode_pick_tick_slots_f32(self, vals, args, B, n, ids, pos, step, req, left, ring, stop, hist, emb, emb_rs, D,
                                       x_next, stream):
        if B == 0:
            return 0
        if not (vals and args and ids and pos and step and left and ring > 0):
            return -1
        return self._tick(_greedy_pick(vals, args, B, n), B, ids, pos, step, stop, hist, emb, emb_rs, D, x_next,
                          left=left, ring=ring)

    def pdn_decode_sample_tick_slots_f32(self, logits, rs, B, V, params, ids, pos, step, req, left, ring, stop, hist, emb,
                                         emb_rs, D, x_next, stream):
        if B == 0:
            return 0
        if not (logits and params and ids and pos and step and req and left and ring > 0):
            return -1
        return self._sample_tick(logits, rs, B, V, params, np.array(flat(req, B, np.int32)), ids, pos, step, stop, hist,
                                 emb, emb_rs, D, x_next, left=left, ring=ring)

    def pdn_kv_store_slots_f32(self, src, src_bs, dst, dst_bs, n_tensors, n_inputs, Ls, D, slots, lens, start, n_rows,
                               max_len, stream):
        if n_tensors == 0 or n_inputs == 0 or Ls == 0:
            return 0
        if not (src and dst and slots and lens and D > 0 and src_bs >= 0 and dst_bs >= max_len * D):
            return -1
        S = flat(src, n_tensors, np.int64)
        Dt = flat(dst, n_tensors, np.int64)
        sl, ln = flat(slots, n_inputs, np.int32), flat(lens, n_inputs, np.int32)
        s0 = flat(start, n_inputs, np.int32) if start else np.zeros(n_inputs, np.int32)
        for j in range(n_tensors):
            for i in range(n_inputs):
                row, a = int(sl[i]), int(s0[i])
                n = min(int(ln[i]), Ls, max_len - a)
                if row < 0 or row >= n_rows or a < 0 or n <= 0:
                    continue
                out = flat(int(Dt[j]) + 4 * (row * dst_bs + a * D), n * D)
                out[...] = flat(int(S[j]) + 4 * i * src_bs, n * D)
        self._count(30)
        return 0

    # -- the wide step ------------------------------------------------------------------------------------------------
    def pdn_decode_wide_supported(self, B, D, H, hd, F, V, max_len):
        return int(9 <= B <= 256 and H > 0 and hd * H == D and hd % 4 == 0 and hd <= 256 and D % 4 == 0 and F > 0
                   and F % 4 == 0 and 0 < V <= 1 << 23 and 0 < max_len and max_len * 4 <= 60 * 1024)

    def pdn_decode_wide_blocks(self, N):
        return -(-N // TN) if N > 0 else 0

    def pdn_decode_wide_work_floats(self, B, K, N):
        return 0                          # (the emulated product needs no workspace)

    def pdn_decode_wide_gemm_f32(self, x, x_rs, mode, norm_w, eps, ns, hd, W, w_rs, blk_cols, w_bs, bias, y, y_rs, epi,
                                 cand_v, cand_i, pos, B, K, N, work, stream):
        if B == 0 or N == 0:
            return 0
        if not (x and W and y and 0 < B <= 256 and K % 4 == 0 and N % blk_cols == 0 and 0 <= mode <= 3 and 0 <= epi <= 2):
            return -1
        width = {0: K, 1: K, 2: 2 * K, 3: ns * (K // max(hd, 1)) * (4 + hd)}[mode]
        X = np.array(view(x, (B, width), (x_rs, 1), np.float32))
        nb = N // blk_cols
        Wm = np.concatenate([np.array(view(W + 4 * j * w_bs, (K, blk_cols), (w_rs, 1), np.float32)) for j in range(nb)],
                            axis=1)
        out = gemm_np(X, mode, flat(norm_w, K) if norm_w else None, eps, ns, hd, Wm,
                      np.array(flat(bias, N)) if bias else None, K)
        live = np.array(flat(pos, B, np.int32)) >= 0 if pos else np.ones(B, bool)
        Y = view(y, (B, N), (y_rs, 1), np.float32)
        Y[live] = (Y[live] + out[live]) if epi == 1 else out[live]
        if epi == 2:
            v, a = candidates(out)
            nbk = -(-N // TN)
            flat(cand_v, B * nbk).reshape(B, nbk)[live] = v[live]
            flat(cand_i, B * nbk, np.int32).reshape(B, nbk)[live] = a[live]
        self._count(31)
        return 0

    def _counted_wide(self, rc):
        self._count(31)
        return rc

    def pdn_decode_wide_pick_tick_rows_f32(self, vals, args, B, n, ids, pos, step, arrive, stop, hist, emb, emb_rs, D,
                                           x_next, stream):
        return self._counted_wide(self.pdn_decode_pick_tick_rows_f32(vals, args, B, n, ids, pos, step, stop, hist, emb,
                                                                     emb_rs, D, x_next, stream))

    def pdn_decode_wide_pick_tick_slots_f32(self, vals, args, B, n, ids, pos, step, arrive, req, left, ring, stop, hist,
                                            emb, emb_rs, D, x_next, stream):
        return self._counted_wide(self.pdn_decode_pick_tick_slots_f32(vals, args, B, n, ids, pos, step, req, left, ring,
                                                                      stop, hist, emb, emb_rs, D, x_next, stream))

    def pdn_decode_wide_sample_tick_rows_f32(self, logits, rs, B, V, params, ids, pos, step, arrive, stop, hist, emb,
                                             emb_rs, D, x_next, stream):
        return self._counted_wide(self.pdn_decode_sample_tick_rows_f32(logits, rs, B, V, params, ids, pos, step, stop,
                                                                       hist, emb, emb_rs, D, x_next, stream))

    def pdn_decode_wide_sample_tick_slots_f32(self, logits, rs, B, V, params, ids, pos, step, arrive, req, left, ring,
                                              stop, hist, emb, emb_rs, D, x_next, stream):
        return self._counted_wide(self.pdn_decode_sample_tick_slots_f32(logits, rs, B, V, params, ids, pos, step, req,
                                                                        left, ring, stop, hist, emb, emb_rs, D, x_next,
                                                                        stream))
