"""Speculative decoding (`generate_ragged(speculate=k)`: prompt-lookup drafts verified in one target pass, statement
llm/speculative.py, kernels csrc/speculative.hip) and beam search (statement llm/beam.py, kernels csrc/beam.hip) on
the decode engine.  A mixin of llm/llama.py's `Llama`; the plan and the issuer are llm/decode_plan.py's."""
import contextlib
import os

import numpy as np

from ..core import Tensor
from . import beam as beam_np
from . import speculative as spec_np
from .decode_plan import _PERSAMPLE_ENTRIES, _SPEC_ENTRIES
from .sampling import Table


class SearchEngine:
    # -- speculative decoding (generate_ragged(speculate=k)): prompt-lookup drafts verified in one target pass
    #    (statement: llm/speculative.py) --------------------------------------------------------------------------------
    def _speculate(self, rows, n, k, sampling, stops):
        """The generator of `generate_ragged(..., speculate=k)`: the prompt pass of `_generate_ragged`, then target passes
        until every row has its tokens; step i is yielded once every live row has its token i (rows run ahead of each
        other).  HIP with the library's speculative entries (`_spec_begin`): one graph-replayed pass per target pass,
        drafted and settled on the device.  Every other path drafts on the host and verifies through the one-token rows
        step (`_spec_host`)."""
        if n == 0:
            return
        lens = np.array([r.size for r in rows], np.int64)
        first = self._prompt_rows(rows, lens, sampling)
        dev = first.device
        R = spec_np.Rows(rows, first.numpy().reshape(-1), n, stops)
        self.last_speculation = R.stats
        yield first
        if not R.live().any():
            return
        hip = self._fast_path(dev)
        st = self._spec_begin(R, k, sampling) if hip else None
        passes = self._spec_device(st, R) if st is not None else self._spec_host(R, k, sampling, hip)
        out = None
        if dev.is_hip:                                   # (the steps handed out: mapped host memory the host fills)
            from .. import hipnp as hp
            out = hp.Mailbox(n, (len(rows), 1), unset=np.iinfo(np.int64).min)
        try:
            i = 1
            while True:
                while R.live().any() and R.ready() <= i:
                    next(passes)
                if i >= R.ready():
                    return
                if out is None:
                    yield Tensor(R.step(i), dtype=np.int64, device=dev)
                else:
                    out.host[i] = R.step(i)
                    yield Tensor(out.slot(i), dtype=np.int64, device=dev, copy=False)
                i += 1
        finally:
            passes.close()

    def _spec_host(self, R, k, sampling, hip):
        """The statement path: per pass, the drafts of llm/speculative.py on the host, then the fed tokens through the
        one-token rows step, query j of every row at once (`_step_module_rows`; the generic rows step on HIP)."""
        dev = self.tok_embedding.weight.device
        while True:
            fed = R.plan(k)
            picks = [[] for _ in fed]
            for j in range(max(len(f) for f in fed)):
                ids = np.array([[f[j] if len(f) > j else 0] for f in fed], np.int64)
                pos = np.array([R.pos[b] + j if len(f) > j else -1 for b, f in enumerate(fed)], np.int64)
                if hip:
                    from .. import hipnp as hp
                    got = self._decode_step_generic_rows(hp.asarray(ids), pos.astype(np.int32), sampling).get()
                else:
                    got = self._step_module_rows(Tensor(ids, dtype=np.int64, device=dev), pos, sampling).numpy()
                for b, f in enumerate(fed):
                    if len(f) > j:
                        picks[b].append(int(got.reshape(-1)[b]))
            R.finish(fed, picks)
            yield

    def _spec_ok(self, B, k):
        """Whether the library provides the speculative pass and takes this model with B (k + 1) query rows."""
        from .. import _lib
        L, D, H, F, V = _lib.lib(), self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        cache_len = self.layers[0].attention.cache_k.shape[1]
        return bool(type(self).wide_decode and B * (k + 1) <= 256 and all(_lib.provides(n) for n in _SPEC_ENTRIES)
                    and L.query("pdn_decode_mixed_supported", D, H, D // H, F, V, cache_len))

    def _spec_begin(self, R, k, sampling):
        """The plan of the speculative pass (buffers, weight views, its graph), kept across calls while the model's arrays
        and (B, k, sampling) stay; then this run's row state uploaded.  None when the library or the model's layout
        refuses it.  `sampling` a llm/sampling.Table: a parameter block per row and the pdnq_ verify tick (include/
        pdn_persample.h); None when the library lacks those entries."""
        from .. import hipnp as hp, _lib
        B = len(R.out)
        per_row = isinstance(sampling, Table)
        if not self._spec_ok(B, k) or (per_row and not all(_lib.provides(n) for n in _PERSAMPLE_ENTRIES)):
            return None
        D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        cache_len = self.layers[0].attention.cache_k.shape[1]
        ns = int(os.environ.get("PDN_DECODE_SPLITS", "0")) or (1 if cache_len <= 256 else 4)
        if ns > 8:
            return None
        key = (B, k, bool(sampling), hp._state["device"], ns, cache_len, tuple(self._weight_ptrs()))
        key += ("per_row",) if per_row else ()
        st = getattr(self, "_spec_st", None)
        if st is not None and st["pending"]:
            hp.synchronize()                             # (an abandoned run's passes: done before its buffers change)
            st["pending"] = 0
        if st is None or st["key"] != key:
            if st is not None and st["graph"]:
                st["graph"].destroy()
            self._spec_st = st = None
            packs = []
            for layer in self.layers:
                a, f = layer.attention, layer.ffn
                qkv = hp.stacked_view([a.Q.weight.data, a.K.weight.data, a.V.weight.data])
                gu = hp.stacked_view([f.gate.weight.data, f.up.weight.data])
                if qkv is None or gu is None or not (a.O.weight.data.is_contiguous() and f.down.weight.data.is_contiguous()):
                    return None
                packs.append((qkv, gu))
            if not (self.lm_head.weight.data.is_contiguous() and self.tok_embedding.weight.data.is_contiguous()):
                return None
            L, K1 = _lib.lib(), k + 1
            Rq, hw = B * K1, min(cache_len, self.freqs_cos.shape[0])
            work = max(L.query("pdn_decode_wide_work_floats", Rq, a, b)
                       for a, b in ((D, 3 * D), (D, D), (F, D), (D, 2 * F), (D, V)))
            nblk = L.query("pdn_decode_wide_blocks", V)
            st = {"key": key, "B": B, "k": k, "R": Rq, "ns": ns, "hw": hw, "packs": packs, "graph": None, "nograph": False,
                  "pending": 0, "sampling": bool(sampling), "params_val": None, "per_row": per_row,
                  "work": hp.zeros((max(work, 4),), np.float32),
                  "cand_v": hp.empty((Rq, nblk), np.float32), "cand_i": hp.empty((Rq, nblk), np.int32),
                  "logits": hp.empty((Rq, V), np.float32), "params": hp.zeros((B, 3) if per_row else (3,), np.int64),
                  # the rows' state (written before a run, then only by the device): history, its length, the position
                  # of the next pass, the budget; the pass counter and the address of the run's mailbox
                  "hist": hp.zeros((B, hw), np.int32), "hlen": hp.zeros((B,), np.int32), "pos": hp.zeros((B,), np.int32),
                  "left": hp.zeros((B,), np.int32), "step": hp.zeros((1,), np.int32), "mbox_ptr": hp.zeros((1,), np.int64),
                  "stop": hp.zeros((-(-V // 32),), np.int32),
                  # the pass's layout, made by the draft kernel
                  "tok": hp.zeros((Rq,), np.int64), "qpos": hp.zeros((Rq,), np.int32), "runs": hp.zeros((B, 4), np.int32),
                  "picks": hp.zeros((Rq,), np.int64),
                  **{n: hp.zeros((Rq, w), np.float32) for n, w in
                     (("x", D), ("qkv", 3 * D), ("att", ns * H * (4 + D // H)), ("gu", 2 * F))}}
            self._spec_st = st
        hist = np.zeros((B, st["hw"]), np.int32)
        for b, h in enumerate(R.hist):
            hist[b, :h.size] = h
        st["hist"][...] = hist
        st["hlen"][...] = np.array([h.size for h in R.hist], np.int32)
        st["pos"][...] = R.pos.astype(np.int32)
        st["left"][...] = R.left.astype(np.int32)
        st["step"][...] = np.int32(0)
        st["stop"][...] = self._stop_mask(R.stops)
        # one mailbox slot per pass: a pass moves every live row at least one token on, so n - 1 passes finish the run
        st["mbox"] = hp.Mailbox(max(int(R.left.max()), 1), (B, k + 4), unset=np.iinfo(np.int64).min)
        st["mbox_ptr"][...] = np.int64(st["mbox"]._ptr)
        self._run_values(st, sampling)
        return st

    def _spec_launches(self, st):
        """One target pass: the draft kernel, the embedding rows of the fed tokens, the mixed step's layers on the B (k + 1)
        query rows, the vocabulary projection (block candidates, or full logit rows when sampling) and the verify tick."""
        from .. import hipnp as hp, _lib
        L, s = _lib.lib(), hp.stream()
        D, V, B, k, Rq = self.embed_dim, self.vocab_size, st["B"], st["k"], st["R"]
        emb = self.tok_embedding.weight.data
        p = {n: st[n]._ptr for n in ("hist", "hlen", "pos", "left", "tok", "qpos", "runs", "picks", "stop", "step",
                                     "mbox_ptr", "x", "work", "logits", "cand_v", "cand_i")}
        L.call("pdn_spec_draft_rows", p["hist"], st["hw"], p["hlen"], p["pos"], p["left"], B, k, p["tok"], p["qpos"],
               p["runs"], s)
        L.call("pdn_embedding_gather_f32", emb._ptr, V, D, emb._strides[0], p["tok"], Rq, p["x"], hp.err_flag_ptr(), s)
        self._mixed_layers(st, st["packs"], B, k + 1, Rq, st["ns"], s)
        head, bias = self.lm_head, self._head_bias()
        full = st["sampling"]
        cv, ci = (None, None) if full else (p["cand_v"], p["cand_i"])
        L.call("pdn_decode_wide_gemm_f32", p["x"], D, 1, self.norm.weight.data._ptr, self.norm.eps, 0, 0,
               head.weight.data._ptr, V, V, 0, bias, p["logits"], V, 0 if full else 2, cv, ci, p["qpos"], Rq, D, V,
               p["work"], s)
        row = (p["tok"], p["qpos"], B, k, p["picks"], p["hist"], st["hw"], p["hlen"], p["pos"], p["left"], p["stop"],
               p["step"], p["mbox_ptr"], s)
        if full:
            L.call("pdnq_spec_verify_sample_tick_f32" if st["per_row"] else "pdn_spec_verify_sample_tick_f32", p["logits"], V,
                   V, st["params"]._ptr, *row)
        else:
            L.call("pdn_spec_verify_pick_tick_f32", p["cand_v"], p["cand_i"], st["cand_v"].shape[1], *row)

    def _spec_issue(self, st):
        """Queue one target pass; the first one of a plan captures its graph (whose two real runs work on a copy of the
        row state and a scratch mailbox: the state is put back afterwards, `_issue`)."""
        self._issue(st, "graph", lambda: self._spec_launches(st), dict.fromkeys(("hist", "hlen", "pos", "left", "step")),
                    redirect=("mbox_ptr", st["mbox"], 2), gather=False, graphs=st)
        st["pending"] += 1

    def _spec_device(self, st, R):
        """The device path: passes queued back to back (one ahead of the one being read when `decode_ahead`), each read
        from its mailbox slot [count, drafted, accepted, tokens...] per row.  A pass is queued only while some live row
        may still need it: its budget exceeds the passes already queued for it."""
        from .. import hipnp as hp
        B, k = st["B"], st["k"]
        try:
            while True:
                depth = 2 if type(self).decode_ahead else 1
                while st["pending"] < depth and (R.live() & (R.left > st["pending"])).any():
                    self._spec_issue(st)
                if not st["pending"]:
                    raise RuntimeError("speculative decoding: no pass left to read")
                got = np.array(st["mbox"].slot(R.stats["passes"]).get()).reshape(B, k + 4)
                st["pending"] -= 1
                R.stats["passes"] += 1
                for b in range(B):
                    c = int(got[b, 0])
                    if c > 0:
                        y = got[b, 3:3 + c]
                        R.take(b, y, int(got[b, 1]), int(got[b, 2]), bool(np.isin(y[-1], R.stops)))
                yield
        finally:
            if st["pending"]:
                hp.synchronize()
                st["pending"] = 0

    def _beam_module(self, rows, n, W, lp, stops):
        """The NumPy statement on the tape-node operators (the `cpu` device, training mode, fast_decode = False): logits of
        `_step_logits_rows`, top-k / select of llm/beam.py, the cache reorder by indexing."""
        G, B = len(rows), len(rows) * W
        lens = np.array([r.size for r in rows], np.int64)
        dev = self.tok_embedding.weight.device
        caches = [c for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)]
        z = np.asarray(self._prefill_rows(rows, np.arange(G) * W).numpy(), np.float32)
        hist = np.zeros((n, B, 2), np.int64)
        fins = [[] for _ in range(G)]
        scores = np.zeros(B, np.float32)
        pos = np.repeat(lens, W)                      # (the position just fed: the prompt's pass counts as len)
        ids = np.zeros(B, np.int64)
        last = 0
        for s in range(n):
            if s:
                logits = self._step_logits_rows(Tensor(ids.reshape(B, 1), dtype=np.int64, device=dev), pos)
                z = np.asarray(logits.numpy(), np.float32)
            cl, ci, sl = beam_np.topk_rows(z, W, stops)
            parent = np.arange(B)
            for g in range(G):
                r0 = g * W
                if pos[r0] < 0:
                    continue
                k, nb = (slice(g, g + 1), 1) if s == 0 else (slice(r0, r0 + W), W)
                tok, par, sc, fin = beam_np.select_group(scores[r0:r0 + W], cl[k], ci[k], sl[k].reshape(nb, stops.size),
                                                         stops, W, first=s == 0)
                hist[s, r0:r0 + W, 0], hist[s, r0:r0 + W, 1] = tok, par
                scores[r0:r0 + W], ids[r0:r0 + W] = sc, tok
                fins[g] += [(s, p, t, raw) for p, t, raw in fin]
                if len(fins[g]) >= W:
                    pos[r0:r0 + W] = -1
                else:
                    pos[r0:r0 + W] += 1
                    parent[r0:r0 + W] = r0 + par
            last = s
            move = np.flatnonzero((parent != np.arange(B)) & (pos > 0))
            for c in caches:                          # (every source read before any row is written)
                src = [c.data[int(parent[r]), :int(pos[r])].copy() for r in move]
                for r, v in zip(move, src):
                    c.data[int(r), :int(pos[r])] = v
            if (pos < 0).all():
                break
        live = [None if pos[g * W] < 0 else scores[g * W:(g + 1) * W] for g in range(G)]
        return beam_np.results(hist[:last + 1], fins, live, last, W, lp)

    def _beam_buffers(self, B, W, S, n_hist):
        """Device state of a beam search over B = G * W rows (csrc/beam.hip): candidates, scores, parents, the (token,
        parent beam) history of n_hist steps, the finished lists, the counters and the live-group mailbox."""
        from .. import hipnp as hp
        caches = [c.data for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)]
        G = B // W
        return dict(W=W, S=S, n_hist=n_hist, cand_lp=hp.empty((B, W), np.float32), cand_id=hp.empty((B, W), np.int32),
                    stop_lp=hp.empty((B, max(S, 1)), np.float32), stops=hp.zeros((max(S, 1),), np.int32),
                    scores=hp.zeros((B,), np.float32), parent=hp.zeros((B,), np.int32),
                    arrive=hp.zeros((1,), np.int32), live_acc=hp.zeros((1,), np.int32),
                    hist=hp.zeros((n_hist, B, 2), np.int32), fin_n=hp.zeros((G,), np.int32),
                    fin=hp.zeros((G, 2 * W - 1, 4), np.int32), live=hp.Mailbox(n_hist, (1,), unset=np.iinfo(np.int64).min),
                    caches=hp.asarray(np.array([c._ptr for c in caches], np.int64)), n_caches=len(caches),
                    cache_bs=caches[0]._strides[0], cache_len=caches[0].shape[1])

    def _beam_launches(self, bm, logits, rs, pos, step, ids, x, first):
        """top-k -> select -> KV-cache reorder of one beam step over the logit rows at `logits` (first: the B / W prompt
        rows of the prompt pass)."""
        from .. import hipnp as hp, _lib
        L, s = _lib.lib(), hp.stream()
        W, S, V, D = bm["W"], bm["S"], self.vocab_size, self.embed_dim
        B = bm["scores"].shape[0]
        emb = self.tok_embedding.weight.data
        cl, ci, sl, stops = (bm[k]._ptr for k in ("cand_lp", "cand_id", "stop_lp", "stops"))
        L.call("pdn_beam_topk_rows_f32", logits, rs, B, V, W, int(first), pos, stops, S, cl, ci, sl, s)
        L.call("pdn_beam_select_f32", cl, ci, sl, stops, S, B // W, W, int(first), bm["scores"]._ptr, ids,
               bm["parent"]._ptr, pos, step, bm["arrive"]._ptr, bm["live_acc"]._ptr, bm["hist"]._ptr, bm["n_hist"],
               bm["fin_n"]._ptr, bm["fin"]._ptr, bm["live"]._ptr, bm["n_hist"], emb._ptr, emb._strides[0], D, x, s)
        L.call("pdn_kv_reorder_rows_f32", bm["caches"]._ptr, bm["n_caches"], bm["cache_bs"], B, bm["cache_len"], D,
               bm["parent"]._ptr, pos, s)

    def _beam_device(self, rows, n, W, lp, stops):
        """beam_search on a HIP device: the prompt pass (`_prefill_rows`, into rows g * W) and its beam launches, then one
        decode step per generated token -- a replay of the captured beam plan (or, where the plan refuses the shapes, the
        generic per-row step and the beam launches one by one).  The host polls the live-group count of each step,
        queuing the next step first; at the end it reads the history and backtracks."""
        from .. import hipnp as hp
        G, B = len(rows), len(rows) * W
        lens = np.array([r.size for r in rows], np.int64)
        st = self._decode_plan(B, ragged=True, beam=W, n_stops=stops.size)
        if st is not None:
            bm, pos, step, ids, x = st["bm"], st["pos"], st["step"], st["ids"], st["x"]
        else:
            bm = self._beam_buffers(B, W, stops.size, n + 2)
            pos, step, ids, x = hp.zeros((B,), np.int32), hp.zeros((1,), np.int32), hp.zeros((B, 1), np.int64), None
        bm["live"].host[...] = bm["live"].unset
        if stops.size:
            bm["stops"][...] = stops.astype(np.int32)
        bm["scores"][...] = np.float32(0)
        bm["fin_n"][...] = np.int32(0)
        step[...] = np.int32(0)
        pos[...] = np.repeat(lens, W).astype(np.int32)
        logits = self._prefill_rows(rows, np.arange(G) * W).data
        if not logits.is_contiguous():
            logits = logits.copy()
        self._beam_launches(bm, logits._ptr, self.vocab_size, pos._ptr, step._ptr, ids._ptr, x._ptr if x is not None else None,
                            first=True)
        last = 0
        live = int(bm["live"].slot(0).get().reshape(-1)[0])
        queued = False
        for s in range(1, n):
            if live == 0:
                break
            top = int(lens.max()) + s
            if st is None:
                p = pos.get().astype(np.int32)
                self._decode_step_generic_rows(ids, p)
                ws = self._decode_ws_rows
                self._beam_launches(bm, ws["logits"]._ptr, self.vocab_size, pos._ptr, step._ptr, ids._ptr, None, False)
            else:
                if not queued:
                    self._beam_issue(st, top)
                queued = s + 1 < n and self._beam_ahead(st, top + 1)
            last = s
            live = int(bm["live"].slot(s).get().reshape(-1)[0])
        hp.synchronize()                                 # (a step queued ahead: all its rows had stopped)
        hist = bm["hist"].get()[:last + 1].astype(np.int64)
        fin_n, fin, sc, p = bm["fin_n"].get(), bm["fin"].get(), bm["scores"].get(), pos.get()
        fins = [[(int(e[0]), int(e[1]), int(e[2]), np.int32(e[3]).view(np.float32)) for e in fin[g, :fin_n[g]]]
                for g in range(G)]
        live_sc = [None if p[g * W] < 0 else sc[g * W:(g + 1) * W] for g in range(G)]
        return beam_np.results(hist, fins, live_sc, last, W, lp)

    def _beam_issue(self, st, top):
        """Issue the next step of a beam plan (its furthest row at position `top`); captures its graph first when this
        range count has none.  The capture's two real runs see every row stopped -- no cache, score or history is
        written -- and the rows' state is put back afterwards (`_issue`)."""
        @contextlib.contextmanager
        def stopped():
            k = int(st["step"].get()[0])
            st["pos"][...] = np.int32(-1)
            yield
            live = st["bm"]["live"]
            live.host[k:min(k + 2, live.n)] = live.unset         # (the capture's runs counted no live group there)
        self._issue_step(st, top, dict.fromkeys(("ids", "pos", "step")), around=stopped)

    def _beam_ahead(self, st, top):
        """Queue the next beam step right behind the issued one if its graph exists (decode_ahead); True if queued."""
        return bool(type(self).decode_ahead and self._issue_step(st, top))
