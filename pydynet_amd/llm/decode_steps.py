"""The steps of Llama generation, one new token per row: the graph-replayed step of `generate` / `generate_ragged`
(`_decode_step_hip`, `_decode_step_rows`: the plan and the issuer of llm/decode_plan.py), the same step from the
library's generic entry points for models the plan refuses, and the step on the tape-node operators (the `cpu` device,
training mode, other dtypes) -- with the prompt passes and the generators that drive them.  A mixin of llm/llama.py's
`Llama`."""
import numpy as np

from ..core import Tensor
from . import logit_edits as edit_np
from . import logprobs as lp_np
from . import penalties as pen_np
from . import stop_sequences as ss_np
from . import token_fsm as fsm_np
from .decode_plan import _EDIT_ENTRIES, _FSM_ENTRIES, _PEN_ENTRIES
from .sampling import Table, draw_rows, params_buffer, sample_next, sample_next_table


class DecodeSteps:
    def _generate(self, input_ids, max_new_tokens, sampling, penalty=None, n_lp=None, edit=None, fsm=None):
        B, L = input_ids.shape
        next_id = None
        pen = None
        # (the rows' requests and prompt lengths: llm/logit_edits.py)
        erows = None if edit is None else edit_np.Rows(B, edit, np.arange(B), np.full(B, L))
        # (the rows' machines, states and prompt lengths: llm/token_fsm.py)
        frows = None if fsm is None else fsm_np.Rows(B, fsm, np.arange(B), np.full(B, L))
        if penalty is not None:                                   # (the rows' prompts and counts: llm/penalties.py)
            ids = np.asarray(input_ids.numpy() if isinstance(input_ids, Tensor) else input_ids).reshape(B, L)
            pen = pen_np.Rows(B, self.vocab_size, penalty, list(ids))
        for i, pos in enumerate(range(L, max_new_tokens)):
            if i == 0:
                logits = self(input_ids, 0)[:, -1, :]             # prompt pass: fills the KV caches
                if pen is not None:
                    logits = self._penalize_prompt(logits, pen.prompts, penalty)
                if frows is not None:
                    logits = self._fsm_rows(logits, fsm, frows.start_state)
                if erows is not None:
                    logits = self._edit_rows(logits, edit, erows.req, np.zeros(B, np.int64))
                next_id = logits.argmax(-1, True) if sampling is None else sample_next(logits, pos, *sampling)
                lp = None if n_lp is None else self._logprobs_rows(logits, next_id.numpy(), n_lp)
            elif self._fast_path(next_id.device):
                # (`more`: another token will be asked for -- the step after this one may be queued ahead)
                out = self._decode_step_hip(next_id.data, pos, more=pos + 1 < max_new_tokens, sampling=sampling,
                                            pen=pen, n_lp=n_lp, edit=erows, fsm=frows)
                out, lp = out if n_lp is not None else (out, None)
                next_id = Tensor(out, dtype=np.int64, device=next_id.device, copy=False)
            else:
                logits = self(next_id, pos)[:, -1, :]
                if pen is not None:
                    logits = self._penalize_step(logits, pen, next_id.numpy(), np.full(B, pos))
                if frows is not None:
                    logits = self._fsm_step_host(logits, frows, next_id.numpy(), np.full(B, pos))
                if erows is not None:
                    logits = self._edit_step_host(logits, erows, np.full(B, pos))
                next_id = logits.argmax(-1, True) if sampling is None else sample_next(logits, pos, *sampling)
                lp = None if n_lp is None else self._logprobs_rows(logits, next_id.numpy(), n_lp)
            yield next_id if n_lp is None else (next_id, lp_np.as_step(lp))

    def _logprobs_rows(self, logits, tokens, n):
        """llm/logprobs.py on logit rows (R, V) (a Tensor or a device array) and the tokens (R,) they yielded (< 0: none).
        On a HIP device: pdn_logprobs_rows_f32 (csrc/logprobs.hip); on `cpu` the statement.  Returns Logprobs of host
        arrays: token (R,), top_ids / top_logprobs (R, n)."""
        from .. import _lib
        x = logits.data if isinstance(logits, Tensor) else logits
        tokens = np.asarray(tokens.get() if hasattr(tokens, "get") else tokens, np.int64).reshape(-1)
        if not getattr(getattr(logits, "device", None), "is_hip", False) and isinstance(x, np.ndarray):
            return lp_np.rows(x.reshape(tokens.size, -1), tokens, n)
        from .. import hipnp as hp
        V = self.vocab_size
        x = x.reshape(tokens.size, V) if len(x.shape) != 2 else x
        if x.dtype != np.float32 or x._strides[1] != 1 or x._strides[0] < V:
            x = x.astype(np.float32).copy() if x.dtype != np.float32 else x.copy()
        R = tokens.size
        tok, ids, top = (hp.empty((R,), np.float32), hp.empty((R, max(n, 1)), np.int64),
                         hp.empty((R, max(n, 1)), np.float32))
        step = 65535                                              # (rows per call: the grid's second dimension)
        L = _lib.lib()
        work = hp.zeros((L.query("pdn_logprobs_work_bytes", min(R, step), V, n) // 8 + 2,), np.int64)
        for r0 in range(0, R, step):
            r1 = min(R, r0 + step)
            t = hp.asarray(tokens[r0:r1])
            L.call("pdn_logprobs_rows_f32", x._ptr + r0 * x._strides[0] * 4, x._strides[0], r1 - r0, V, n, t._ptr,
                   tok._ptr + r0 * 4, ids._ptr + r0 * max(n, 1) * 8, top._ptr + r0 * max(n, 1) * 4, work._ptr, hp.stream())
        return lp_np.Logprobs(tok.get(), ids.get()[:, :n], top.get()[:, :n])

    def _penalize_prompt(self, logits, prompts, penalty):
        """The logits (A, V) of a prompt pass penalised for prompts[i] (no generated token yet: only the repetition penalty
        of the prompt's tokens acts).  On a HIP device with the library's entries: pdn_penalty_rows_f32 in place (stream
        ordered, no plan); elsewhere the statement of llm/penalties.py."""
        from .. import _lib
        dev, V = logits.device, self.vocab_size
        if dev.is_hip and logits.data.dtype == np.float32 and all(_lib.provides(n) for n in _PEN_ENTRIES):
            from .. import hipnp as hp
            x = logits.data
            if x._strides[1] != 1 or x._strides[0] < V:
                x = x.copy()
            seen, prm = hp.asarray(pen_np.seen_bits(prompts, V)), hp.asarray(pen_np.params_bytes(*penalty))
            _lib.lib().call("pdn_penalty_rows_f32", x._ptr, x._strides[0], x.shape[0], V, prm._ptr, None, seen._ptr, None,
                            None, None, hp.stream())
            return Tensor(x, dtype=np.float32, device=dev, copy=False)
        z = pen_np.penalize(logits.numpy(), np.zeros((len(prompts), V), np.int64), pen_np.seen_rows(prompts, V), *penalty)
        return Tensor(z, dtype=np.float32, device=dev)

    @staticmethod
    def _penalize_step(logits, pen, ids, pos):
        """The statement on a step of a path without the device state (host counts in `pen`, llm/penalties.Rows): the
        generated tokens fed at positions pos (B,) counted, then the (B, V) logits penalised."""
        pen.feed(ids, pos)
        return Tensor(pen.apply(np.asarray(logits.numpy(), np.float32)), dtype=np.float32, device=logits.device)

    def _fsm_rows(self, logits, spec, states, pos=None):
        """The mask of llm/token_fsm.py on logit rows (R, V) (a Tensor or a device array) for rows in the states
        `states` (R,) of `spec` (llm/token_fsm.Machines; -1: off); pos (R,) marks the rows to leave alone (-1; None: none).
        On a HIP device with the library's entries: pdnf_fsm_rows_f32 in place (stream ordered, no plan); elsewhere the
        statement.  Returns what it was given, a Tensor or a device array."""
        from .. import _lib
        V = self.vocab_size
        x = logits.data if isinstance(logits, Tensor) else logits
        states = np.asarray(states, np.int64).reshape(-1)
        if pos is not None:
            states = np.where(np.asarray(pos, np.int64).reshape(-1) >= 0, states, -1)
        if not isinstance(x, np.ndarray) and x.dtype == np.float32 and all(_lib.provides(n) for n in _FSM_ENTRIES):
            from .. import hipnp as hp
            if x._strides[1] != 1 or x._strides[0] < V:
                x = x.copy()
            off, tok, _, dfl = (hp.asarray(a) for a in fsm_np.padded(spec.tables, *spec.caps))
            d_states = hp.asarray(states.astype(np.int32))
            _lib.lib().call("pdnf_fsm_rows_f32", x._ptr, x._strides[0], x.shape[0], V, off._ptr, tok._ptr, dfl._ptr,
                            spec.caps[0], spec.caps[1], d_states._ptr, None, None, None, hp.stream())
            return Tensor(x, dtype=np.float32, device=logits.device, copy=False) if isinstance(logits, Tensor) else x
        z = np.asarray(logits.numpy() if isinstance(logits, Tensor) else x.get() if hasattr(x, "get") else x, np.float32)
        z = fsm_np.apply(z, spec.tables, states)
        if isinstance(logits, Tensor):
            return Tensor(z, dtype=np.float32, device=logits.device)
        if isinstance(x, np.ndarray):
            return z
        x[...] = z
        return x

    def _fsm_step_host(self, logits, frows, ids, pos):
        """`_fsm_rows` on a step of a path without the device state (`frows`: llm/token_fsm.Rows): every row's state
        advanced by the token it is fed (ids (B,), host or device) at positions pos (B,), -1 for a row that computes nothing."""
        pos = np.asarray(pos, np.int64).reshape(-1)
        ids = np.asarray(ids.get() if hasattr(ids, "get") else ids, np.int64).reshape(-1)
        cur, frows.word = fsm_np.step_states(frows.spec.tables, frows.word, frows.start_state, frows.start, ids, pos)
        return self._fsm_rows(logits, frows.spec, cur, pos)

    def _edit_rows(self, logits, spec, reqs, generated, pos=None):
        """The statement of llm/logit_edits.py on logit rows (R, V) (a Tensor or a device array) for requests reqs[i] of
        `spec` (llm/logit_edits.Edits) that have generated[i] tokens; pos (R,) marks the rows to leave alone (-1; None:
        none).  On a HIP device with the library's entries: pdne_logit_edit_rows_f32 in place (stream ordered, no plan);
        elsewhere the statement.  Returns what it was given, a Tensor or a device array."""
        from .. import _lib
        V = self.vocab_size
        x = logits.data if isinstance(logits, Tensor) else logits
        reqs = np.asarray(reqs, np.int64).reshape(-1)
        generated = np.asarray(generated, np.int64).reshape(-1)
        pos = None if pos is None else np.asarray(pos, np.int64).reshape(-1)
        if not isinstance(x, np.ndarray) and x.dtype == np.float32 and all(_lib.provides(n) for n in _EDIT_ENTRIES):
            from .. import hipnp as hp
            if x._strides[1] != 1 or x._strides[0] < V:
                x = x.copy()
            src = [None if a is None else hp.asarray(a) for a in spec.packed(np.maximum(reqs, 0))]
            prm, gen = hp.asarray(edit_np.params_bytes(spec.m)), hp.asarray(generated.astype(np.int32))
            skip = None if pos is None else hp.asarray(np.where((pos >= 0) & (reqs >= 0), 0, -1).astype(np.int32))
            stop = hp.asarray(self._stop_mask(spec.stops)) if spec.m > 0 else None
            _lib.lib().call("pdne_logit_edit_rows_f32", x._ptr, x._strides[0], x.shape[0], V, prm._ptr,
                            *(None if a is None else a._ptr for a in src), gen._ptr,
                            None if skip is None else skip._ptr, None if stop is None else stop._ptr, None, None,
                            hp.stream())
            return Tensor(x, dtype=np.float32, device=logits.device, copy=False) if isinstance(logits, Tensor) else x
        z = np.asarray(logits.numpy() if isinstance(logits, Tensor) else x.get() if hasattr(x, "get") else x, np.float32)
        live = np.flatnonzero(reqs >= 0 if pos is None else (pos >= 0) & (reqs >= 0))
        z = np.array(z)
        if live.size:
            z[live] = edit_np.apply(z[live], spec.allow_rows(reqs[live]), spec.bias_rows(reqs[live]), generated[live],
                                    spec.m, spec.stops)
        if isinstance(logits, Tensor):
            return Tensor(z, dtype=np.float32, device=logits.device)
        if isinstance(x, np.ndarray):
            return z
        x[...] = z
        return x

    def _edit_step_host(self, logits, erows, pos):
        """`_edit_rows` on a step of a path without the device state (`erows`: llm/logit_edits.Rows): every row's request
        at positions pos (B,), -1 for a row that computes nothing."""
        pos = np.asarray(pos, np.int64).reshape(-1)
        return self._edit_rows(logits, erows.spec, erows.req, np.maximum(pos - erows.start, 0), pos)

    def _generate_ragged(self, rows, n, sampling, stops, penalty=None, n_lp=None, edit=None, fsm=None, stopseq=None):
        B = len(rows)
        lens = np.array([r.size for r in rows], np.int64)
        if n == 0:
            return
        pen = None if penalty is None else pen_np.Rows(B, self.vocab_size, penalty, rows)
        erows = None if edit is None else edit_np.Rows(B, edit, np.arange(B), lens)
        frows = None if fsm is None else fsm_np.Rows(B, fsm, np.arange(B), lens)
        # (the rows' matcher: llm/stop_sequences.py -- every path drops the rows it reports from `live`; the graph path's
        #  device state stops them at the same step, csrc/stop_seq.hip)
        srows = None if stopseq is None else ss_np.Rows(B, stopseq, np.arange(B))
        nxt = self._prompt_rows(rows, lens, sampling, penalty, n_lp, edit, fsm)
        if n_lp is not None:
            nxt, lp = nxt
        live = np.ones(B, bool)
        if stops.size:
            live = ~np.isin(nxt.numpy().reshape(-1), stops)
        if srows is not None:
            live = live & ~srows.feed(nxt.numpy().reshape(-1))
        yield nxt if n_lp is None else (nxt, lp_np.as_step(lp))
        fast = self._fast_path(nxt.device)
        if fast:
            from .. import hipnp as hp
            # tokens by STEP: slot i holds step i of every row (-1 for a stopped row), so "not written yet" is its own
            # value; two slots beyond the last step for the runs of a graph capture
            run = {"lens": lens, "live": live, "sampling": sampling, "stop_mask": self._stop_mask(stops), "pen": pen,
                   "edit": erows, "fsm": frows, "stopseq": srows,
                   "hist": hp.Mailbox(n + 2, (B, 1), unset=np.iinfo(np.int64).min), "lp": n_lp}
        ids = nxt.data
        for i in range(1, n):
            if not live.any():
                return
            if fast:
                run["live"] = live
                ids = self._decode_step_rows(ids, run, i, more=i + 1 < n)
                ids, lp = ids if n_lp is not None else (ids, None)
                nxt = Tensor(ids, dtype=np.int64, device=nxt.device, copy=False)
            else:
                nxt = self._step_module_rows(nxt, np.where(live, lens + i, -1), sampling, pen=pen, n_lp=n_lp,
                                             edit=erows, fsm=frows)
                nxt, lp = nxt if n_lp is not None else (nxt, None)
            if stops.size or srows is not None:
                yield nxt if n_lp is None else (nxt, lp_np.as_step(lp))
                tok = nxt.numpy().reshape(-1)                    # (fast path: a poll of the mapped history slot)
                live = live & (tok >= 0) & ~np.isin(tok, stops)
                if srows is not None:
                    live = live & ~srows.feed(tok)
                continue
            yield nxt if n_lp is None else (nxt, lp_np.as_step(lp))

    def _prompt_rows(self, rows, lens, sampling, penalty=None, n_lp=None, edit=None, fsm=None):
        """The prompt pass of a ragged generation: the prompts right-padded to the longest and run as one batched
        causal pass from position 0 (no real token attends to a pad after it); each row's logits at its last real token,
        gathered before lm_head.  The cache slots the pads wrote, [len_b, L_max) of row b, are put back as they were: a
        row's cache is written at its own positions only.  `penalty`: the logits penalised for each row's prompt first;
        `fsm` (llm/token_fsm.Machines): then masked for request b's start state; `edit` (llm/logit_edits.Edits): then
        edited for request b in row b.
        Returns the first token of every row, (B, 1) int64 (`n_lp`: and their Logprobs)."""
        B, Lm, lo = len(rows), int(lens.max()), int(lens.min())
        ids = np.zeros((B, Lm), np.int64)
        for b, r in enumerate(rows):
            ids[b, :r.size] = r
        caches = [c for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)]
        saved = [c.data[:B, lo:Lm].copy() for c in caches] if lo < Lm else []
        dev = self.tok_embedding.weight.device
        h = self._forward_hidden(Tensor(ids, dtype=np.int64, device=dev), 0)
        last = h.reshape(B * Lm, self.embed_dim)[np.arange(B) * Lm + lens - 1].reshape(B, 1, self.embed_dim)
        logits = self.lm_head(last)[:, -1, :]
        for c, keep in zip(caches, saved):
            for b in np.flatnonzero(lens < Lm):
                c.data[int(b), int(lens[b]):Lm] = keep[int(b), int(lens[b]) - lo:]
        if penalty is not None:
            logits = self._penalize_prompt(logits, rows, penalty)
        if fsm is not None:
            logits = self._fsm_rows(logits, fsm, fsm.start_states(np.arange(B)))
        if edit is not None:
            logits = self._edit_rows(logits, edit, np.arange(B), np.zeros(B, np.int64))
        nxt = logits.argmax(-1, True) if sampling is None else draw_rows(logits, lens, sampling, np.arange(B))
        if n_lp is None:
            return nxt
        return nxt, self._logprobs_rows(logits, nxt.numpy(), n_lp)

    def _step_module_rows(self, ids, pos, sampling, req=None, pen=None, n_lp=None, edit=None, fsm=None):
        """One ragged decode step on the tape-node operators (the `cpu` device, fast_decode = False, training mode,
        other dtypes): row b's token at position pos[b] (-1: a stopped row, which yields -1).  The NumPy statement of what
        the per-row kernels compute.  `req`: the counter id of each row (Llama.serve; default: the row).  `pen`
        (llm/penalties.Rows): the fed tokens counted and the logits penalised before the pick.  `edit`
        (llm/logit_edits.Rows): then the rows' edits; `fsm` (llm/token_fsm.Rows): between the two, the rows' machines
        advanced by the fed tokens and their masks.  `n_lp`: returns (ids,
        Logprobs of the rows, none for rows at -1)."""
        p = np.maximum(pos, 0)
        logits = self._step_logits_rows(ids, pos)
        if pen is not None:
            logits = self._penalize_step(logits, pen, ids.numpy(), pos)
        if fsm is not None:
            logits = self._fsm_step_host(logits, fsm, ids.numpy(), pos)
        if edit is not None:
            logits = self._edit_step_host(logits, edit, pos)
        # (`sampling` a llm/sampling.Table: row b with the values of the request it holds)
        nxt = logits.argmax(-1, True) if sampling is None else draw_rows(
            logits, p, sampling, np.arange(len(p)) if req is None else req, rows=req)
        if pos.min() < 0:
            out = nxt.numpy().reshape(-1, 1)
            out[pos < 0] = -1
            nxt = Tensor(out, dtype=np.int64, device=ids.device)
        if n_lp is None:
            return nxt
        return nxt, self._logprobs_rows(logits, nxt.numpy(), n_lp)

    def _step_logits_rows(self, ids, pos):
        """The logits (B, V) of `_step_module_rows`' step: row b fed ids[b] at position pos[b] (-1: stopped)."""
        tok = ids.data if pos.min() >= 0 else np.maximum(ids.numpy(), 0)      # (a stopped row's -1 is no token)
        h = self.tok_embedding(Tensor(tok, dtype=np.int64, device=ids.device) if tok is not ids.data else ids)
        for layer in self.layers:
            h = layer.step_rows(h, pos, self.freqs_cos, self.freqs_sin)
        return self.lm_head(self.norm(h))[:, -1, :]

    def _decode_step_hip(self, ids, pos: int, more: bool = False, sampling=None, pen=None, n_lp=None, edit=None,
                         fsm=None):
        """One decode step (one new token per sequence) without building tape nodes.  ids: (B, 1) int64
        device array; returns the next ids, (B, 1) int64.  The step is ONE hipGraph replay: norm + projection,
        RoPE + cache append, decode attention, SwiGLU + down projection and the greedy pick all read the position
        from device memory (csrc/decode.hip), so nothing changes between replays but the data.  `sampling`: None =
        greedy, else (temperature, top_k, top_p, seed) and the step ends in the sample tick (csrc/sample.hip).  `pen`
        (llm/penalties.Rows of this generation, or None): a penalty plan; its rows are reset from the prompts when a new
        generation begins.  `edit` (llm/logit_edits.Rows of this generation, or None): an edit plan, reset likewise; `fsm` (llm/token_fsm.Rows of this generation, or None): an FSM plan.
        `n_lp`: returns (ids, Logprobs of the step)."""
        from .. import hipnp as hp
        B = ids.shape[0]
        cache = self.layers[0].attention.cache_k
        limit = min(cache.shape[1], self.freqs_cos.shape[0])
        # raw pointers / device-side offsets are formed from `pos`: refuse what the module path would also refuse
        # (the reference fails with a NumPy broadcast error, model.py:105-110)
        if pos < 0 or pos >= limit:
            raise ValueError(f"decode position {pos} is outside the KV cache / RoPE table "
                             f"(max_seq_len {cache.shape[1]}, {self.freqs_cos.shape[0]} RoPE rows)")
        if B > cache.shape[0]:
            raise ValueError(f"batch {B} exceeds the KV cache's max_batch_size {cache.shape[0]}")
        st = self._decode_plan(B, sampling is not None, penalty=pen is not None, n_lp=n_lp, edit=edit is not None,
                               fsm=False if fsm is None else fsm.spec.caps)
        if st is None:
            return self._decode_step_generic(ids, pos, sampling, pen, n_lp, edit, fsm)
        ahead, st["ahead"] = st.get("ahead"), None
        if ahead is not None:
            if (ahead[0] == pos and ahead[1] is ids and st["params_val"] == sampling     # exactly this step, queued ahead
                    and st.get("pen_run") is pen and st.get("edit_run") is edit and st.get("fsm_run") is fsm):
                out = st["last_out"] = ahead[2]
                if more and pos + 1 < limit:
                    self._decode_ahead(st, pos + 1)
                return out if n_lp is None else (out, self._lp_read(st, pos))
            hp.synchronize()                                     # a different request: the queued step is void
            st["host_pos"] = st["last_out"] = None               # (position and ids are uploaded again below)
        if st["host_pos"] != pos:
            st["pos"][...] = np.int32(pos)                       # (later steps: the device advances it itself)
            if st["rows"]:                                       # (the wide step: equal positions, history by step)
                st["step"][...] = np.int32(pos)
                st["stop"][...] = np.int32(0)
            # a new generation: its own history -- slots in mapped host memory the pick kernel stores into directly
            st["hist"] = hp.Mailbox(cache.shape[1], (B, 1))
            self._hist_begin(st, st["hist"])
        self._run_values(st, sampling, pen, edit, fsm)
        if ids is not st["ids"] and ids is not st.get("last_out"):
            st["ids"][...] = ids                                 # (not the array the previous step returned: that
            self._decode_gather(st)                              # one's embedding row is already in x)
        # (a capture's two runs write the cache rows of positions pos and pos + 1: both must exist)
        keep = {"pos": np.int32(pos), **({"step": np.int32(pos)} if st["rows"] else {}), "ids": None}
        self._issue_step(st, pos, keep, redirect=("hist_ptr", st["hist"]), capture=pos + 2 < limit)
        st["host_pos"] = pos + 1
        # the caller's own array = this position's slot of the history (host memory the GPU writes): reading the token
        # polls THAT slot only -- no copy command, no event -- while the compute stream may already run the next step
        out = st["last_out"] = st["hist"].slot(pos)
        if more and pos + 1 < limit:
            self._decode_ahead(st, pos + 1)
        return out if n_lp is None else (out, self._lp_read(st, pos))

    def _decode_ahead(self, st, pos):
        """Queue the step of position `pos` right behind the one just issued -- its input ids are already where the
        gather reads them -- so the GPU does not idle while the host hands the previous token to the caller.  The
        result is kept for the next `_decode_step_hip(last_out, pos)` call; any other call discards it.  Nothing is
        queued with decode_ahead off, or while the step's graph is missing (a new range count: the next call captures)."""
        if type(self).decode_ahead and self._issue_step(st, pos):
            st["host_pos"] = pos + 1
            st["ahead"] = (pos, st["last_out"], st["hist"].slot(pos))

    def _eager_ws(self, attr, B, extra=()):
        """The activation rows of an eager step (`extra`: more rows of width D), kept on the model as `attr` while the
        device and the row count stay."""
        from .. import hipnp as hp
        D, F, V = self.embed_dim, self.ffn_dim, self.vocab_size
        ws = getattr(self, attr, None)
        if ws is None or ws["x"].device_index != hp._state["device"] or ws["x"].shape[0] != B:
            ws = {n: hp.empty((B, w), np.float32) for n, w in
                  (("x", D), ("h", D), ("q", D)) + tuple((n, D) for n in extra)
                  + (("att", D), ("g", F), ("u", F), ("sw", F), ("logits", V))}
            setattr(self, attr, ws)
        return ws

    @staticmethod
    def _eager_gemv(B):
        """c (B, N; row stride `ldc`) = beta c + a (B, K) @ w (+ bias) as one skinny `pdn_gemm_f32`."""
        from .. import hipnp as hp, _lib
        L, st = _lib.lib(), hp.stream()

        def gemv(a_ptr, K, w, c_ptr, N, beta=0.0, bias=None, ldc=None):
            wd = w.data
            L.call("pdn_gemm_f32", B, N, K, 1.0, a_ptr, K, 1, wd._ptr, wd._strides[0], wd._strides[1], beta, c_ptr,
                   N if ldc is None else ldc, bias, 1, 1, 0, 0, 0, 0, 0, 0, None, None, 0, None, 0, st)
        return gemv

    def _eager_ffn(self, layer, ws, gemv):
        """The second half of a layer of an eager step, from the attention output ws["att"]: x += att @ Wo, then
        x += swiglu(RMSNorm(x) @ Wgate, RMSNorm(x) @ Wup) @ Wdown."""
        from .. import hipnp as hp, _lib
        L, st = _lib.lib(), hp.stream()
        D, F, B = self.embed_dim, self.ffn_dim, ws["x"].shape[0]
        x, h, att, g, u, sw = (ws[n]._ptr for n in ("x", "h", "att", "g", "u", "sw"))
        f = layer.ffn
        gemv(att, D, layer.attention.O.weight, x, D, beta=1.0)        # x += att @ Wo
        L.call("pdn_rmsnorm_fwd_f32", x, layer.post_attn_norm.weight.data._ptr, h, None, B, D,
               layer.post_attn_norm.eps, st)
        gemv(h, D, f.gate.weight, g, F)
        gemv(h, D, f.up.weight, u, F)
        L.call("pdn_swiglu_fwd_f32", g, u, sw, B * F, st)
        gemv(sw, F, f.down.weight, x, D, beta=1.0)                    # x += swiglu @ Wdown

    def _eager_tail(self, ws, gemv, fed, pos, pen, draw, n_lp, edit=None, fsm=None):
        """The end of an eager step: the final RMSNorm and the vocabulary projection; `pen` (llm/penalties.Rows): the
        statement of llm/penalties.py on the host counts, the tokens `fed` (device ids) at positions `pos` (host (B,), -1:
        a stopped row) counted first; `fsm` (llm/token_fsm.Rows): the rows' machines advanced by `fed` and their masks
        (`_fsm_step_host`); `edit` (llm/logit_edits.Rows): the rows' edits (`_edit_rows`); then the greedy
        pick, or `draw(out)`, which launches the draw into `out`.  Returns
        the ids, (B, 1) int64 (`n_lp`: and the rows' Logprobs, none for rows at -1)."""
        from .. import hipnp as hp, _lib
        D, V, B = self.embed_dim, self.vocab_size, ws["x"].shape[0]
        _lib.lib().call("pdn_rmsnorm_fwd_f32", ws["x"]._ptr, self.norm.weight.data._ptr, ws["h"]._ptr, None, B, D,
                        self.norm.eps, hp.stream())
        gemv(ws["h"]._ptr, D, self.lm_head.weight, ws["logits"]._ptr, V, bias=self._head_bias())
        if pen is not None:
            pen.feed(fed.get(), pos)
            ws["logits"][...] = pen.apply(ws["logits"].get())
        if fsm is not None:
            self._fsm_step_host(ws["logits"], fsm, fed, pos)     # (contiguous rows: in place)
        if edit is not None:
            self._edit_step_host(ws["logits"], edit, pos)        # (contiguous rows: in place)
        if draw is None:
            out = ws["logits"].argmax(-1, keepdims=True)
        else:
            out = hp.empty((B, 1), np.int64)
            draw(out)
        if n_lp is None:
            return out
        tok = np.array(out.get()).reshape(-1)
        tok[pos < 0] = -1
        return out, self._logprobs_rows(ws["logits"], tok, n_lp)

    def _decode_step_generic(self, ids, pos: int, sampling=None, pen=None, n_lp=None, edit=None, fsm=None):
        """The same step from the library's generic entry points (skinny `pdn_gemm_f32`, RMSNorm, RoPE, decode
        attention, SwiGLU), ~77 launches from preallocated buffers: for shapes / layouts the graph path does not take."""
        from .. import hipnp as hp, _lib
        L, st = _lib.lib(), hp.stream()
        D, H, V = self.embed_dim, self.n_heads, self.vocab_size
        hd, half = D // H, D // H // 2
        B = ids.shape[0]
        ws = self._eager_ws("_decode_ws", B)
        gemv = self._eager_gemv(B)
        x, h, q, att = (ws[n]._ptr for n in ("x", "h", "q", "att"))
        emb = self.tok_embedding.weight.data
        idc = ids if ids.is_contiguous() else ids.copy()
        L.call("pdn_embedding_gather_f32", emb._ptr, V, D, emb._strides[0], idc._ptr, B, x, hp.err_flag_ptr(), st)
        cos = self.freqs_cos.data._ptr + pos * half * 4
        sin = self.freqs_sin.data._ptr + pos * half * 4
        for layer in self.layers:
            a = layer.attention
            ck, cv = a.cache_k.data, a.cache_v.data
            cbs = ck._strides[0]                                          # floats between sequences in the cache
            kslot, vslot = ck._ptr + pos * D * 4, cv._ptr + pos * D * 4   # row b of the slot is cbs floats further
            L.call("pdn_rmsnorm_fwd_f32", x, layer.input_norm.weight.data._ptr, h, None, B, D, layer.input_norm.eps, st)
            gemv(h, D, a.Q.weight, q, D)
            gemv(h, D, a.K.weight, kslot, D, ldc=cbs)
            gemv(h, D, a.V.weight, vslot, D, ldc=cbs)
            L.call("pdn_rope_f32", q, cos, sin, q, B, 1, H, hd, 0, st)
            for b in range(B):
                L.call("pdn_rope_f32", kslot + b * cbs * 4, cos, sin, kslot + b * cbs * 4, 1, 1, H, hd, 0, st)
            L.call("pdn_attention_decode_f32", q, ck._ptr, cv._ptr, att, B, H, pos + 1, hd, cbs, st)
            self._eager_ffn(layer, ws, gemv)

        def draw(out):                                # (the sampled form of the pick: counter (pos, b))
            L.call("pdn_sample_rows_f32", ws["logits"]._ptr, V, B, V, params_buffer(*sampling)._ptr, pos, out._ptr, st)
        return self._eager_tail(ws, gemv, ids, np.full(B, pos), pen, None if sampling is None else draw, n_lp, edit, fsm)

    # -- ragged decode (generate_ragged): every row at its own position ------------------------------
    def _decode_step_rows(self, ids, run, i: int, more: bool = False):
        """Step i >= 1 of a ragged generation: row b's token at position lens[b] + i, rows the host knows to have stopped
        at -1.  ids: (B, 1) int64 device array (the previous step's tokens); returns this step's tokens, (B, 1) int64, -1
        for rows stopped before it.  The graph path of `_decode_step_hip` with the *_rows_f32 launches: the positions, the
        step counter and the stop bitmask live on the device, the history is indexed by the step (`run["hist"]`), and the
        range count follows the furthest row, max_b lens[b] + i, which the host knows without a device read."""
        from .. import hipnp as hp
        lens, live, sampling = run["lens"], run["live"], run["sampling"]
        B, top = len(lens), int(lens.max()) + i
        cache = self.layers[0].attention.cache_k
        limit = min(cache.shape[1], self.freqs_cos.shape[0])
        pos = np.where(live, lens + i, -1).astype(np.int32)
        n_lp = run.get("lp")
        st = self._decode_plan(B, sampling is not None, ragged=True, penalty=run.get("pen") is not None, n_lp=n_lp,
                               edit=run.get("edit") is not None, per_row=isinstance(sampling, Table),
                               fsm=False if run.get("fsm") is None else run["fsm"].spec.caps,
                               stopseq=False if run.get("stopseq") is None else run["stopseq"].spec.caps)
        if st is None:
            out = self._decode_step_generic_rows(ids, pos, sampling, pen=run.get("pen"), n_lp=n_lp, edit=run.get("edit"),
                                                 fsm=run.get("fsm"))
            out, lp = out if n_lp is not None else (out, None)
            if pos.min() < 0:
                tok = out.get().reshape(B, 1)
                tok[pos < 0] = -1
                out = hp.asarray(tok)
            return out if n_lp is None else (out, lp)
        ahead, st["ahead"] = st.get("ahead"), None
        if ahead is not None:
            if ahead[0] == (id(run), i) and ahead[1] is ids and st["run"] is run:   # exactly this step, queued ahead
                out = st["last_out"] = ahead[2]
                if more and top + 1 < limit:
                    self._decode_ahead_rows(st, run, i + 1)
                return out if n_lp is None else (out, self._lp_read(st, i))
            hp.synchronize()                                     # a different request: the queued step is void
            st["host_step"] = st["last_out"] = None
        if st["run"] is not run or st["host_step"] != i:
            st["run"] = run                                      # (later steps: the device advances pos and step itself)
            st["pos"][...] = pos
            st["step"][...] = np.int32(i)
            st["stop"][...] = run["stop_mask"]
            self._hist_begin(st, run["hist"])
        self._run_values(st, sampling, run.get("pen"), run.get("edit"), run.get("fsm"), run.get("stopseq"), lens)
        if ids is not st["ids"] and ids is not st.get("last_out"):
            # (a stopped row's -1 is no token: any valid id stands in, its row computes nothing that is kept)
            st["ids"][...] = np.maximum(ids.get(), 0) if isinstance(ids, hp.readback_array) else ids
            self._decode_gather(st)
        self._issue_step(st, top, {"pos": pos, "step": np.int32(i), "ids": None}, redirect=("hist_ptr", run["hist"]),
                         capture=top + 2 < limit)
        st["host_step"] = i + 1
        out = st["last_out"] = run["hist"].slot(i)
        if more and top + 1 < limit:
            self._decode_ahead_rows(st, run, i + 1)
        return out if n_lp is None else (out, self._lp_read(st, i))

    def _decode_ahead_rows(self, st, run, i):
        """`_decode_ahead` for a ragged plan: queue step i right behind the one just issued."""
        if type(self).decode_ahead and self._issue_step(st, int(run["lens"].max()) + i):
            st["host_step"] = i + 1
            st["ahead"] = ((id(run), i), st["last_out"], run["hist"].slot(i))

    def _decode_step_generic_rows(self, ids, pos, sampling=None, req=None, pen=None, n_lp=None, edit=None, fsm=None):
        """`_decode_step_generic` with a position per row (pos: host int32, -1 = a stopped row: computed at position 0,
        no cache slot written): k / v are projected into scratch rows and written to each row's own slot, RoPE takes
        each row's own cos / sin row, and the attention runs over each row's own key count (pdn_attention_decode_rows_f32).
        `req` (Llama.serve): the counter id of each row, drawn by the slot tick (default: the row).  `pen`
        (llm/penalties.Rows): the statement of the penalties on the host counts.  `edit` (llm/logit_edits.Rows): the rows'
        edits.  Returns the ids of every row, (B, 1)
        int64 (`n_lp`: and the rows' Logprobs, none for rows at -1)."""
        from .. import hipnp as hp, _lib
        L, st = _lib.lib(), hp.stream()
        D, H, V = self.embed_dim, self.n_heads, self.vocab_size
        hd, half = D // H, D // H // 2
        B = ids.shape[0]
        p = np.maximum(pos, 0)
        ws = self._eager_ws("_decode_ws_rows", B, ("k", "v"))
        if "lens" not in ws:
            ws["lens"] = hp.zeros((B,), np.int32)
        ws["lens"][...] = (p + 1).astype(np.int32)
        gemv = self._eager_gemv(B)
        x, h, q, k, v, att, logits = (ws[n]._ptr for n in ("x", "h", "q", "k", "v", "att", "logits"))
        emb = self.tok_embedding.weight.data
        idc = ids if ids.is_contiguous() else ids.copy()
        if pos.min() < 0:                                                 # (a stopped row's -1 is no token)
            idc = hp.asarray(np.maximum(idc.get(), 0))
        L.call("pdn_embedding_gather_f32", emb._ptr, V, D, emb._strides[0], idc._ptr, B, x, hp.err_flag_ptr(), st)
        cos, sin = self.freqs_cos.data._ptr, self.freqs_sin.data._ptr
        for layer in self.layers:
            a = layer.attention
            ck, cv = a.cache_k.data, a.cache_v.data
            cbs = ck._strides[0]                                          # floats between sequences in the cache
            L.call("pdn_rmsnorm_fwd_f32", x, layer.input_norm.weight.data._ptr, h, None, B, D, layer.input_norm.eps, st)
            gemv(h, D, a.Q.weight, q, D)
            gemv(h, D, a.K.weight, k, D)
            gemv(h, D, a.V.weight, v, D)
            for b in range(B):
                row, ang = b * D * 4, int(p[b]) * half * 4
                L.call("pdn_rope_f32", q + row, cos + ang, sin + ang, q + row, 1, 1, H, hd, 0, st)
                if pos[b] >= 0:
                    slot = (b * cbs + int(p[b]) * D) * 4
                    L.call("pdn_rope_f32", k + row, cos + ang, sin + ang, ck._ptr + slot, 1, 1, H, hd, 0, st)
                    L.call("pdn_memcpy_d2d", cv._ptr + slot, v + row, D * 4, st)
            L.call("pdn_attention_decode_rows_f32", q, ck._ptr, cv._ptr, att, B, H, ws["lens"]._ptr, int(p.max()) + 1,
                   hd, cbs, st)
            self._eager_ffn(layer, ws, gemv)

        def draw(out):                                # (counter (pos[b], b): the per-row tick on scratch copies)
            if isinstance(sampling, Table):           # (a block per row: the per-row standalone entry, or the statement)
                rq = np.arange(B) if req is None else np.asarray(req, np.int64).reshape(B)
                dev = self.tok_embedding.weight.device
                got = sample_next_table(Tensor(ws["logits"], dtype=np.float32, device=dev, copy=False), p, sampling, rq, rq)
                out[...] = got.data
                return
            pd, step = hp.asarray(p.astype(np.int32)), hp.zeros((1,), np.int32)
            if req is not None:                       # (counter (pos[b], req[b]): the slot tick, a budget of one token)
                rq, left = hp.asarray(np.asarray(req, np.int32).reshape(B)), hp.asarray(np.ones(B, np.int32))
                L.call("pdn_decode_sample_tick_slots_f32", logits, V, B, V, params_buffer(*sampling)._ptr, out._ptr,
                       pd._ptr, step._ptr, rq._ptr, left._ptr, 1, None, None, None, 0, 0, None, st)
            else:
                L.call("pdn_decode_sample_tick_rows_f32", logits, V, B, V, params_buffer(*sampling)._ptr, out._ptr,
                       pd._ptr, step._ptr, None, None, None, 0, 0, None, st)
        return self._eager_tail(ws, gemv, idc, pos, pen, None if sampling is None else draw, n_lp, edit, fsm)
