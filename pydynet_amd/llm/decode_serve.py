"""The engine of `Llama.serve` (continuous batching): the scheduler and the prompt pass that admits requests, the served
plan on the graph path (steps issued, queued ahead and read in order through a history ring), chunked prefill on the
mixed step (csrc/extend.hip; schedule: llm/chunked.py) and the prefix cache (llm/prefix.py).  A mixin of llm/llama.py's
`Llama`; the plan and the issuer are llm/decode_plan.py's."""
import numpy as np

from ..core import Tensor
from . import chunked
from . import logit_edits as edit_np
from . import logprobs as lp_np
from . import penalties as pen_np
from . import prefix as prefix_np
from . import stop_sequences as ss_np
from . import token_fsm as fsm_np
from .decode_plan import _MIXED_ENTRIES
from .sampling import Table, draw_rows


class ServeEngine:
    def _serve(self, rows, budgets, S, sampling, stops, penalty=None, n_lp=None, edit=None, fsm=None, stopseq=None):
        """The scheduler of `serve`.  Per step: the rows holding a request decode one token, then the rows freed by the
        previous step take the waiting requests in order through one prompt pass (`_serve_prefill`), then the step is
        yielded.  The host keeps, per row, the request, the position of its next decode step, the tokens it may still
        produce and its last token; on the graph path the device keeps the same in the served plan (`_serve_begin`) and
        the host writes it only after an admission, when every queued step has been read.  `edit` (llm/logit_edits.Edits):
        request r's edits follow it into the row that takes it, as its prompt set and counts do with penalties; `fsm`
        (llm/token_fsm.Machines): likewise request r's machine, from its start state.  `stopseq`
        (llm/stop_sequences.StopSeqs): a request also ends at the end of one of its stop sequences -- the host matcher
        (`srows`) reports it on every path, from the tokens it reads, and on the graph path the device stops the row in
        the same step (csrc/stop_seq.hip), so a step queued ahead computes nothing for it."""
        lens = np.array([r.size for r in rows], np.int64)
        queue = [r for r in range(len(rows)) if budgets[r] > 0]   # FIFO by index; a budget of 0 never takes a row
        req = np.full(S, -1, np.int64)
        pos = np.full(S, -1, np.int64)
        left = np.zeros(S, np.int64)
        last = np.zeros(S, np.int64)
        hip = self._fast_path(self.tok_embedding.weight.device)
        st = self._serve_begin(S, sampling, stops, penalty, n_lp, edit, fsm, stopseq) if hip else None  # None: the plan refuses -> generic
        pen = None if penalty is None or st is not None else pen_np.Rows(S, self.vocab_size, penalty)   # (host counts)
        erows = None if edit is None or st is not None else edit_np.Rows(S, edit)                        # (host state)
        frows = None if fsm is None or st is not None else fsm_np.Rows(S, fsm)                           # (host state)
        srows = None if stopseq is None else ss_np.Rows(S, stopseq)                                      # (every path)
        q = 0
        try:
            while True:
                run = req >= 0
                adm = np.flatnonzero(~run)[:len(queue) - q]      # the lowest free rows take the lowest waiting requests
                new = np.array(queue[q:q + adm.size], np.int64)
                q += adm.size
                if not run.any() and not adm.size:
                    return
                p = np.where(run, pos, -1)
                toks = np.full(S, -1, np.int64)
                lpv = None if n_lp is None else lp_np.none(S, n_lp)
                if st is not None:
                    # (invariant: at most one step is queued here, and it is this step's -- void if no row runs)
                    if run.any() and not st["pending"]:
                        self._serve_issue(st, int(p.max()))
                    if not adm.size:
                        nxt = np.where(run & (left > 1), p + 1, -1)
                        if nxt.max() >= 0:
                            self._serve_ahead(st, int(nxt.max()))    # the next step, queued before this one is read
                        toks[run] = self._serve_read(st, lpv, run)[run]
                elif run.any():
                    toks[run] = self._serve_step_eager(hip, last, p, req, run, sampling, pen, n_lp, lpv, erows, frows)[run]
                shown = req.copy()
                if adm.size:
                    first = self._serve_prefill([rows[r] for r in new], adm, new, sampling, penalty, n_lp, edit, fsm)
                    if n_lp is not None:
                        first, lpf = first
                        lp_np.merge(lpv, adm, lpf)
                    if pen is not None:
                        pen.reset(adm, [rows[r] for r in new])
                    if erows is not None:
                        erows.reset(adm, new, lens[new])
                    if frows is not None:
                        frows.reset(adm, new, lens[new])
                    if st is not None and st["pending"]:
                        d = self._serve_read(st, lpv, run)       # (stream order: that step ran before the prefill)
                        toks[run] = d[run]
                    toks[adm], shown[adm] = first, new
                    req[adm], pos[adm], left[adm] = new, lens[new], budgets[new]
                    if srows is not None:
                        srows.reset(adm, new)
                # every row that produced a token: one position further, one token less; a request ends at its budget
                # or at a stop id, and its row is free for the next step
                has = shown >= 0
                left[has] -= 1
                pos[has] += 1
                last[has] = toks[has]
                done = has & ((left <= 0) | np.isin(toks, stops))
                if srows is not None:                            # (the admitted rows' first tokens included)
                    done |= has & srows.feed(toks)
                req[done], pos[done], left[done] = -1, -1, 0
                if st is not None and adm.size:
                    self._serve_write(st, req, pos, left, last)
                    if st["pen"]:                                # (no step queued: after every step of the old request)
                        self._pen_reset(st, adm, [rows[r] for r in new], penalty)
                    if st["edit"]:
                        self._edit_reset(st, adm, new, lens[new], edit)
                    if st["fsm"]:
                        self._fsm_reset(st, adm, new, lens[new], fsm)
                    if st["stopseq"]:
                        self._stop_reset(st, adm, stopseq.sets_of(new), lens[new], first, stopseq)
                    if (req >= 0).any():
                        self._serve_ahead(st, int(np.where(req >= 0, pos, -1).max()))
                yield (shown, toks) if n_lp is None else (shown, toks, lpv)
        finally:
            if st is not None and st["pending"]:
                from .. import hipnp as hp
                hp.synchronize()                                 # (queued steps store into this run's history)
                st["pending"] = 0

    def _serve_step_eager(self, hip, last, p, req, on, sampling, pen, n_lp, lpv, edit=None, fsm=None):
        """One decode step of the served rows off the graph path: rows `on` (bool) fed their last tokens `last` at
        positions `p` (-1: a row that does not decode) with the counter ids `req` -- the generic rows step on a HIP device
        (`hip`), the tape-node step elsewhere.  Returns the tokens of every row, host (S,); `n_lp`: the records of rows
        `on` are merged into `lpv`."""
        ids, rq = last.reshape(-1, 1), np.maximum(req, 0)
        if hip:
            from .. import hipnp as hp
            out = self._decode_step_generic_rows(hp.asarray(ids), p.astype(np.int32), sampling, rq, pen=pen, n_lp=n_lp,
                                                 edit=edit, fsm=fsm)
        else:
            dev = self.tok_embedding.weight.device
            out = self._step_module_rows(Tensor(ids, dtype=np.int64, device=dev), p, sampling, rq, pen=pen, n_lp=n_lp,
                                         edit=edit, fsm=fsm)
        if n_lp is not None:
            out, lpr = out
            lp_np.merge(lpv, np.flatnonzero(on), lp_np.Logprobs(*(a[on] for a in lpr)))
        return (out.get() if hip else out.numpy()).reshape(-1)

    def _serve_prefill(self, prompts, rows, reqs, sampling, penalty=None, n_lp=None, edit=None, fsm=None):
        """Admit requests `reqs` (their prompts) into decode rows `rows`: the prompts right-padded to the longest run as one
        batched causal pass from position 0 into a staging cache (the layers' caches point at it meanwhile), then
        pdn_kv_store_slots_f32 puts prompt i's keys / values, positions [0, len_i), into cache row rows[i] and zeroes
        position len_i there -- the slot a decode step attends to but never writes (`generate`'s step at position p feeds
        the token of position p - 1), which in a fresh cache holds zeros.  No pad position and no other row is written.
        `penalty`: the logits penalised for each prompt first; `fsm` (llm/token_fsm.Machines): then masked for each
        request's start state; `edit` (llm/logit_edits.Edits): then edited for each
        request (no token generated yet).  Returns the first token of each request (counter (len_i,
        reqs[i]) when sampled; `sampling` a llm/sampling.Table: with request reqs[i]'s own values, through the per-row
        standalone entry), host int64 (`n_lp`: and their Logprobs)."""
        logits = self._prefill_rows(prompts, rows)
        if penalty is not None:
            logits = self._penalize_prompt(logits, prompts, penalty)
        if fsm is not None:
            logits = self._fsm_rows(logits, fsm, fsm.start_states(reqs))
        if edit is not None:
            logits = self._edit_rows(logits, edit, reqs, np.zeros(len(prompts), np.int64))
        lens = np.array([p.size for p in prompts], np.int64)
        first = logits.argmax(-1, True) if sampling is None else draw_rows(logits, lens, sampling, reqs, rows=reqs)
        first = np.asarray(first.numpy()).reshape(-1).astype(np.int64)
        return first if n_lp is None else (first, self._logprobs_rows(logits, first, n_lp))

    def _prefill_rows(self, prompts, rows):
        """The prompt pass of `_serve_prefill` (and of `beam_search`): prompt i's keys / values into cache row rows[i],
        positions [0, len_i), position len_i zeroed.  Returns the logits of each prompt's last real position, (A, V)."""
        A = len(prompts)
        lens = np.array([p.size for p in prompts], np.int64)
        Lp = int(lens.max())
        ids = np.zeros((A, Lp), np.int64)
        for i, p in enumerate(prompts):
            ids[i, :p.size] = p
        dev = self.tok_embedding.weight.device
        caches = [c for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)]
        Bc, T, H, hd = caches[0].shape
        keep = [c.data for c in caches]
        with dev:
            staged = [dev.xp.zeros((A, Lp, H, hd), c.dtype) for c in keep]
        try:
            for c, s in zip(caches, staged):
                c.data = s
            h = self._forward_hidden(Tensor(ids, dtype=np.int64, device=dev), 0)
        finally:
            for c, k in zip(caches, keep):
                c.data = k
        last = h.reshape(A * Lp, self.embed_dim)[np.arange(A) * Lp + lens - 1].reshape(A, 1, self.embed_dim)
        logits = self.lm_head(last)[:, -1, :]
        D = H * hd
        if dev.is_hip and keep[0].dtype == np.float32 and all(k.is_contiguous() for k in keep):
            from .. import hipnp as hp, _lib
            L, s = _lib.lib(), hp.stream()
            src = hp.asarray(np.array([a._ptr for a in staged], np.int64))
            dst = hp.asarray(np.array([k._ptr for k in keep], np.int64))
            zero = hp.zeros((D,), np.float32)
            slots, ln, one = (hp.asarray(np.asarray(a, np.int32)) for a in (rows, lens, np.ones(A)))
            L.call("pdn_kv_store_slots_f32", src._ptr, Lp * D, dst._ptr, keep[0]._strides[0], len(keep), A, Lp, D,
                   slots._ptr, ln._ptr, None, Bc, T, s)
            zeros = hp.asarray(np.full(len(keep), zero._ptr, np.int64))
            L.call("pdn_kv_store_slots_f32", zeros._ptr, 0, dst._ptr, keep[0]._strides[0], len(keep), A, 1, D,
                   slots._ptr, one._ptr, ln._ptr, Bc, T, s)
        else:
            with dev:
                for k, a in zip(keep, staged):
                    for i, b in enumerate(rows):
                        k[int(b), :int(lens[i])] = a[i, :int(lens[i])]
                        if lens[i] < T:
                            k[int(b), int(lens[i])] = 0
        return logits

    # (graph path of `serve`: the served plan holds the rows' state on the device; steps are issued, queued ahead and
    #  read in order, through a ring of `ring` history slots)
    def _serve_begin(self, S, sampling, stops, penalty=None, n_lp=None, edit=None, fsm=None, stopseq=None):
        from .. import hipnp as hp
        st = self._decode_plan(S, sampling is not None, ragged=True, serve=True, penalty=penalty is not None, n_lp=n_lp,
                               edit=edit is not None, per_row=isinstance(sampling, Table),
                               fsm=False if fsm is None else fsm.caps,
                               stopseq=False if stopseq is None else stopseq.caps)
        if st is None:
            return None
        st["table"] = sampling if st["per_row"] else None        # (the rows' blocks: written with their requests)
        if st["pending"]:
            hp.synchronize()                                     # (an abandoned run's queued steps)
        st["hist"] = hp.Mailbox(st["ring"], (S, 1), unset=np.iinfo(np.int64).min)
        self._hist_begin(st, st["hist"])
        st["stop"][...] = self._stop_mask(stops)
        st["pos"][...] = np.full(S, -1, np.int32)
        st["step"][...] = np.int32(0)
        st["left"][...] = np.zeros(S, np.int32)
        st["req"][...] = np.zeros(S, np.int32)
        self._run_values(st, sampling)
        if penalty is not None:                                  # (every row is reset when it takes a request)
            self._pen_reset(st, [], [], penalty)
        if edit is not None:                                     # (likewise: here only min_new_tokens is uploaded)
            self._edit_reset(st, [], [], [], edit)
            st["edit_run"] = None
        if fsm is not None:                                      # (likewise: here only the tables are uploaded)
            self._fsm_reset(st, [], [], [], fsm)
            st["fsm_run"] = None
        if stopseq is not None:                                  # (likewise: the tables and min_new_tokens)
            self._stop_reset(st, [], [], [], None, stopseq)
            st["ss_run"] = None
        st["pending"], st["read"] = 0, 0
        return st

    def _serve_issue(self, st, top):
        """Issue the next decode step of a served plan (its furthest row at position `top`); captures its graph first
        when this range count has none -- the capture's two real runs store into a scratch history and the rows' state
        is put back afterwards (`_issue`)."""
        if self._decode_st is not st:
            raise RuntimeError("another generation replaced the plan of a running serve() on this model")
        self._issue_step(st, top, dict.fromkeys(("ids", "pos", "step", "left")), redirect=("hist_ptr", st["hist"]))
        st["pending"] += 1

    def _serve_ahead(self, st, top):
        """Queue the next step right behind the issued ones (decode_ahead), if its graph exists (a new range count is
        captured when next issued): a row that ends in the step before computes nothing that is kept (its position is -1
        on the device by then)."""
        if type(self).decode_ahead and self._issue_step(st, top):
            st["pending"] += 1

    def _serve_read(self, st, lpv=None, rows=None):
        """The tokens of the oldest unread step, (B,) host int64 (-1 for rows that computed nothing): a poll of its
        mapped history slot, which is then marked unwritten for the step `ring` steps later.  Plans with logprobs: the
        step's records too, rows `rows` (bool) of them merged into `lpv`."""
        h, i = st["hist"], st["read"] % st["ring"]
        tok = np.array(h.slot(i).get()).reshape(-1)
        if st.get("lp_n") is not None:
            # (before the history slot is marked unwritten: the record kernel reads its tokens there)
            lp = self._lp_read(st, st["read"])
            if lpv is not None:
                lp_np.merge(lpv, np.flatnonzero(rows), lp_np.Logprobs(*(a[rows] for a in lp)))
        h.host[i] = h.unset
        st["read"] += 1
        st["pending"] -= 1
        return tok

    def _serve_write(self, st, req, pos, left, last):
        """After an admission (no step queued): the rows' state as the host keeps it -- positions (-1: free), counter
        ids, budgets and last tokens -- written in stream order, and x = the embedding rows of those tokens.  A plan with a
        parameter table: each row's block becomes its request's."""
        st["pos"][...] = pos.astype(np.int32)
        st["req"][...] = np.maximum(req, 0).astype(np.int32)
        if st["table"] is not None:
            self._params_rows(st, st["table"], req)
        st["left"][...] = left.astype(np.int32)
        st["ids"][...] = last.reshape(-1, 1)
        self._decode_gather(st)

    # -- chunked prefill (serve(prefill_chunk=C)): prompts fed C tokens per step (statement: llm/chunked.py) -----------
    def _serve_chunked(self, rows, budgets, S, C, sampling, stops, penalty=None, n_lp=None, prefix=None, edit=None,
                       fsm=None, stopseq=None):
        """The scheduler of `serve` with a chunk: llm/chunked.Schedule decides, per step, which rows decode and which
        prompt tokens are fed.  Graph path (`_mixed_begin`): a step with prompt tokens runs the mixed step (the decode
        rows and the chunks as query rows of the wide product, csrc/extend.hip), a step without runs the served step.
        Every other path decodes as `_serve` does, and a prompt pass runs when the schedule completes prompts: one
        `_serve_prefill` for the requests whose prompts complete in that step.
        `prefix` = k (the prefix cache, llm/prefix.Schedule): on the graph path the rows admitted in a step that reuse
        another row's tokens take them through one copy launch, issued eagerly before the step (`_prefix_copy`), and
        their prefill starts at fed = n; every other path starts every prompt at 0 (the schedule with reuse forced off).
        `stopseq` (llm/stop_sequences.StopSeqs): as in `_serve`; an admitted row's first token comes out of a replayed
        step, so its device tail starts empty."""
        lens = np.array([r.size for r in rows], np.int64)
        hip = self._fast_path(self.tok_embedding.weight.device)
        st = self._mixed_begin(S, C, sampling, stops, penalty, n_lp, edit, fsm, stopseq) if hip else None
        if prefix is None:
            sch = chunked.Schedule(lens, budgets, S, C)
        else:
            sch = prefix_np.Schedule(rows, budgets, S, C, prefix if st is not None else None)
            self.prefix_stats = sch.stats
            if st is not None:
                st.pop("prefix", None)                          # (the cache pointer table: built by the run's first copy)
        pen = None if penalty is None or st is not None else pen_np.Rows(S, self.vocab_size, penalty)   # (host counts)
        erows = None if edit is None or st is not None else edit_np.Rows(S, edit)                        # (host state)
        frows = None if fsm is None or st is not None else fsm_np.Rows(S, fsm)                           # (host state)
        srows = None if stopseq is None else ss_np.Rows(S, stopseq)                                      # (every path)
        dirty = False                                           # (the device's row state differs from the host's)
        try:
            while True:
                if prefix is None:
                    adm, new = sch.admit()
                else:
                    adm, new, don, reuse = sch.admit()
                    if st is not None and adm.size:              # (stream order: after every earlier step of any row)
                        self._prefix_copy(st, sch, adm, don, reuse)
                if adm.size and penalty is not None:            # (stream order: after the steps of the rows' old requests)
                    if st is not None:
                        self._pen_reset(st, adm, [rows[r] for r in new], penalty)
                    else:
                        pen.reset(adm, [rows[r] for r in new])
                if adm.size and edit is not None:               # (likewise)
                    if st is not None:
                        self._edit_reset(st, adm, new, lens[new], edit)
                    else:
                        erows.reset(adm, new, lens[new])
                if adm.size and fsm is not None:                # (likewise)
                    if st is not None:
                        self._fsm_reset(st, adm, new, lens[new], fsm)
                    else:
                        frows.reset(adm, new, lens[new])
                if adm.size and stopseq is not None:            # (likewise; the first token: out of a later step)
                    if st is not None:
                        self._stop_reset(st, adm, stopseq.sets_of(new), lens[new], None, stopseq)
                    srows.reset(adm, new)
                if not sch.busy():
                    return
                n, dec, comp = sch.plan()
                toks = np.full(S, -1, np.int64)
                lpv = None if n_lp is None else lp_np.none(S, n_lp)
                if st is not None:
                    got = np.zeros(S, bool)
                    if st["pending"]:                            # a served step queued ahead: this step's decode rows
                        toks[dec] = self._serve_read(st, lpv, dec)[dec]
                        got |= dec
                    if n.any():
                        inc = dec & ~got
                        self._mixed_issue(st, sch, n, inc, comp, rows)
                        t = self._serve_read(st, lpv, inc | comp)
                        toks[inc | comp] = t[inc | comp]
                        dirty = True
                    elif not got.any() and dec.any():
                        p = np.where(dec, sch.pos, -1)
                        if dirty:
                            self._serve_write(st, sch.req, p, np.where(dec, sch.left, 0), sch.last)
                            dirty = False
                        self._serve_issue(st, int(p.max()))
                        # the next step queued before this one is read, when it is a served step for sure: no prompt
                        # left to feed, and no admission unless a stop id frees a row
                        nxt = np.where(dec & (sch.left > 1), p + 1, -1)
                        if (nxt.max() >= 0 and not (sch.fed < sch.row_lens()).any()
                                and (sch.q >= len(sch.queue) or not (dec & (sch.left <= 1)).any())):
                            self._serve_ahead(st, int(nxt.max()))
                        toks[dec] = self._serve_read(st, lpv, dec)[dec]
                else:
                    if dec.any():
                        toks[dec] = self._serve_step_eager(hip, sch.last, np.where(dec, sch.pos, -1), sch.req, dec,
                                                           sampling, pen, n_lp, lpv, erows, frows)[dec]
                    if comp.any():
                        b = np.flatnonzero(comp)
                        first = self._serve_prefill([rows[r] for r in sch.req[b]], b, sch.req[b], sampling, penalty,
                                                    n_lp, edit, fsm)
                        if n_lp is not None:
                            first, lpf = first
                            lp_np.merge(lpv, b, lpf)
                        toks[b] = first
                shown = sch.finish(n, toks, stops, None if srows is None else srows.feed(toks))
                yield (shown, toks) if n_lp is None else (shown, toks, lpv)
        finally:
            if st is not None and st["pending"]:
                from .. import hipnp as hp
                hp.synchronize()
                st["pending"] = 0

    def _prefix_copy(self, st, sch, adm, donors, reuse):
        """The copies of one step's admissions (llm/prefix.py): rows `adm` take their first `reuse` positions from rows
        `donors`, in every cache tensor, by ONE pdn_kv_copy_prefix_rows_f32 on the decode stream -- outside the captured
        graphs, like `_pen_reset` -- that reads every source as it was before the launch (two admitted rows may take from
        each other).  A row that is its own donor has the data already."""
        from .. import hipnp as hp, _lib
        take = (reuse > 0) & (donors != adm)
        if not take.any():
            return
        P = st.get("prefix")
        if P is None:
            caches = [c.data for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)]
            if not all(c.dtype == np.float32 and c.is_contiguous() for c in caches):
                raise RuntimeError("prefix_cache needs contiguous float32 KV caches")
            P = st["prefix"] = dict(caches=hp.asarray(np.array([c._ptr for c in caches], np.int64)), n=len(caches),
                                    bs=caches[0]._strides[0], rows=caches[0].shape[0], len=caches[0].shape[1])
        # (device copies held until the call has been issued; the allocator orders their reuse on the stream)
        dst, src, ln = (hp.asarray(a[take].astype(np.int32)) for a in (adm, donors, reuse))
        # (the caches as far as the longest copy reaches: the launch is sized by the positions it is given)
        _lib.lib().call("pdn_kv_copy_prefix_rows_f32", P["caches"]._ptr, P["n"], P["bs"], P["rows"],
                        min(P["len"], int(reuse[take].max())), self.embed_dim, dst._ptr, src._ptr, ln._ptr,
                        int(take.sum()), hp.stream())
        sch.stats["launches"] += 1

    def _mixed_ok(self, S, C):
        """Whether the library provides the mixed step and takes this model (any row count up to 256 query rows)."""
        from .. import _lib
        L, D, H, F, V = _lib.lib(), self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        cache_len = self.layers[0].attention.cache_k.shape[1]
        return bool(type(self).wide_decode and S + C <= 256 and all(_lib.provides(n) for n in _MIXED_ENTRIES)
                    and L.query("pdn_decode_mixed_supported", D, H, D // H, F, V, cache_len))

    def _mixed_begin(self, S, C, sampling, stops, penalty=None, n_lp=None, edit=None, fsm=None, stopseq=None):
        """The served plan (`_serve_begin`) plus the buffers of the mixed step (`mixed`), or None when either refuses."""
        from .. import hipnp as hp, _lib
        if not self._mixed_ok(S, C):
            return None
        st = self._serve_begin(S, sampling, stops, penalty, n_lp, edit, fsm, stopseq)
        if st is None or st["ns"] > 8:
            return None
        M = st.get("mixed")
        if M is None or M["C"] != C:
            D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
            R, ns, L = S + C, st["ns"], _lib.lib()
            work = max([L.query("pdn_decode_wide_work_floats", R, k, n) for k, n in ((D, 3 * D), (D, D), (F, D), (D, 2 * F))]
                       + [L.query("pdn_decode_wide_work_floats", S, D, V)])
            nblk = L.query("pdn_decode_wide_blocks", V)
            M = {"C": C, "R": R, "arrive": hp.zeros((1,), np.int32), "work": hp.zeros((max(work, 4),), np.float32),
                 "cand_v": hp.empty((S, nblk), np.float32), "cand_i": hp.empty((S, nblk), np.int32),
                 # the per-step layout (uploaded before each replay): query-row positions (-1: masked), one run per cache
                 # row [first query row, count, start, ends the prompt], the prompt tokens, each slot's emitting row
                 "qpos": hp.zeros((R,), np.int32), "runs": hp.zeros((S, 4), np.int32), "tok": hp.zeros((C,), np.int64),
                 "emit": hp.zeros((S,), np.int64), "xe": hp.empty((S, D), np.float32),
                 **{n: hp.zeros((R, w), np.float32) for n, w in
                    (("x", D), ("qkv", 3 * D), ("att", ns * H * (4 + D // H)), ("gu", 2 * F))}}
            for k in [k for k in st["graphs"] if len(k) > 2 and k[2] == "mixed"]:
                st["graphs"].pop(k).destroy()
            st["mixed"] = M
        return st

    def _mixed_layout(self, st, sch, n, inc, comp, rows):
        """Upload one mixed step: the rows' state (decode rows `inc` at their positions, rows completing their prompt at
        position len for the tick, every other row -1) and the layout of its query rows."""
        M, S, C = st["mixed"], sch.S, sch.C
        lens = sch.row_lens()
        qpos = np.full(S + C, -1, np.int32)
        runs = np.zeros((S, 4), np.int32)
        tok = np.zeros(C, np.int64)
        emit = np.arange(S, dtype=np.int64)
        qpos[:S][inc] = sch.pos[inc]
        for b in np.flatnonzero(inc):
            runs[b] = (b, 1, sch.pos[b], 0)
        q = S
        for b in sorted(np.flatnonzero(n > 0).tolist(), key=lambda b: int(sch.req[b])):
            f, k = int(sch.fed[b]), int(n[b])
            runs[b] = (q, k, f, int(f + k == lens[b]))
            qpos[q:q + k] = np.arange(f, f + k)
            tok[q - S:q - S + k] = rows[int(sch.req[b])][f:f + k]
            emit[b] = q + k - 1
            q += k
        pos = np.where(inc, sch.pos, -1)
        pos[comp] = lens[comp]
        st["pos"][...] = pos.astype(np.int32)
        st["req"][...] = np.maximum(sch.req, 0).astype(np.int32)
        if st["table"] is not None:
            self._params_rows(st, st["table"], sch.req)
        st["left"][...] = np.where(inc | comp, sch.left, 0).astype(np.int32)
        M["qpos"][...] = qpos
        M["runs"][...] = runs
        M["tok"][...] = tok
        M["emit"][...] = emit

    def _mixed_issue(self, st, sch, n, inc, comp, rows):
        """Issue one mixed step (no step queued): upload its layout, capture its graph first when there is none."""
        if self._decode_st is not st:
            raise RuntimeError("another generation replaced the plan of a running serve() on this model")
        self._mixed_layout(st, sch, n, inc, comp, rows)
        ns = st["ns"]
        self._issue(st, (ns, st["sampling"], "mixed", st["mixed"]["C"]), lambda: self._mixed_launches(st, ns),
                    dict.fromkeys(("ids", "pos", "step", "left")), redirect=("hist_ptr", st["hist"]))
        st["pending"] += 1

    def _mixed_launches(self, st, ns):
        """The mixed step: S decode query rows (st["x"]) and C prompt rows (their embedding rows) through the layers on
        the wide product -- q | k | v, the KV append and the extend attention, the output projection (mode 3 merge),
        gate | up, down -- then each slot's emitting row gathered, the vocabulary projection and the wide slot tick on
        the S rows of the served plan."""
        from .. import hipnp as hp, _lib
        L, s = _lib.lib(), hp.stream()
        M = st["mixed"]
        D, V, S, C, R = self.embed_dim, self.vocab_size, st["B"], M["C"], M["R"]
        x, work = M["x"]._ptr, M["work"]._ptr
        emb = self.tok_embedding.weight.data
        L.call("pdn_memcpy_d2d", x, st["x"]._ptr, S * D * 4, s)
        L.call("pdn_embedding_gather_f32", emb._ptr, V, D, emb._strides[0], M["tok"]._ptr, C, x + S * D * 4,
               hp.err_flag_ptr(), s)
        self._mixed_layers(M, st["packs"], S, C, R, ns, s)
        xe = M["xe"]._ptr
        L.call("pdn_embedding_gather_f32", x, R, D, D, M["emit"]._ptr, S, xe, hp.err_flag_ptr(), s)
        full = st["sampling"] or st["pen"] or st["edit"] or st["fsm"]
        cv, ci = (None, None) if full else (M["cand_v"]._ptr, M["cand_i"]._ptr)
        L.call("pdn_decode_wide_gemm_f32", xe, D, 1, self.norm.weight.data._ptr, self.norm.eps, 0, 0,
               self.lm_head.weight.data._ptr, V, V, 0, self._head_bias(), st["logits"]._ptr, V, 0 if full else 2, cv, ci,
               st["pos"]._ptr, S, D, V, work, s)
        # (penalty plans: a row completing its prompt here is at position len = start and counts nothing; greedy: the
        #  plan's candidates are those of the penalty kernel.  Edit plans: that row has generated no token; the
        #  candidates are those of the edit kernel.  FSM plans: that row is in its start state, which the kernel takes at
        #  g = 0 whatever the row's word holds.  Stop sequences: the tick leaves that row at position len + 1, behind its
        #  first generated token, as it leaves a decode row at start + g)
        self._pen_step(st, s)
        self._fsm_step(st, s)
        self._edit_step(st, s)
        self._decode_tick(st, s, mixed=M)
        self._lp_tick(st, s)
        self._stop_step(st, s)

    def _mixed_layers(self, M, packs, n_runs, max_run, R, ns, s):
        """The layers of the mixed step on R query rows (M["x"] in, M["x"] out): q | k | v with RMSNorm in the load, the KV
        append and the extend attention over the runs M["runs"] (n_runs of at most max_run queries), the output
        projection (mode 3 merge), gate | up, down -- every product on the wide kernel, masked by M["qpos"]."""
        from .. import _lib
        L = _lib.lib()
        D, H, F = self.embed_dim, self.n_heads, self.ffn_dim
        hd = D // H
        x, qkv, att, gu, work, qpos, runs = (M[n]._ptr for n in ("x", "qkv", "att", "gu", "work", "qpos", "runs"))
        cos, sin = self.freqs_cos.data._ptr, self.freqs_sin.data._ptr
        max_len = min(self.layers[0].attention.cache_k.shape[1], self.freqs_cos.shape[0])
        for layer, (wqkv, wgu) in zip(self.layers, packs):
            a, f = layer.attention, layer.ffn
            ck, cv = a.cache_k.data, a.cache_v.data
            nrm = layer.input_norm
            L.call("pdn_decode_wide_gemm_f32", x, D, 1, nrm.weight.data._ptr, nrm.eps, 0, 0, wqkv._ptr, D, D,
                   wqkv._strides[0], None, qkv, 3 * D, 0, None, None, qpos, R, D, 3 * D, work, s)
            L.call("pdn_kv_append_rows_f32", qkv, 3 * D, cos, sin, ck._ptr, cv._ptr, ck._strides[0], runs, n_runs, max_run,
                   R, H, hd, max_len, s)
            L.call("pdn_decode_extend_attention_f32", qkv, 3 * D, cos, sin, ck._ptr, cv._ptr, ck._strides[0], runs, n_runs,
                   max_run, R, H, hd, ns, max_len, att, s)
            L.call("pdn_decode_wide_gemm_f32", att, M["att"].shape[1], 3, None, 0.0, ns, hd, a.O.weight.data._ptr, D, D,
                   0, None, x, D, 1, None, None, qpos, R, D, D, work, s)
            nrm = layer.post_attn_norm
            L.call("pdn_decode_wide_gemm_f32", x, D, 1, nrm.weight.data._ptr, nrm.eps, 0, 0, wgu._ptr, F, F,
                   wgu._strides[0], None, gu, 2 * F, 0, None, None, qpos, R, D, 2 * F, work, s)
            L.call("pdn_decode_wide_gemm_f32", gu, 2 * F, 2, None, 0.0, 0, 0, f.down.weight.data._ptr, D, D, 0, None,
                   x, D, 1, None, None, qpos, R, F, D, work, s)
