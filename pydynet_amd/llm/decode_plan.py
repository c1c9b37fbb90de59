"""The graph-replayable Llama decode step (csrc/decode*.hip): its plan dict (`_decode_plan`, kept in `self._decode_st`),
the launches of one step and the ticks that end it, and `_issue`, the one place where a step's hipGraph is captured or
replayed -- every generation feature (generate, generate_ragged, serve, chunked prefill, speculative decoding, beam
search) issues its steps through it.  A mixin of llm/llama.py's `Llama`: the class switches are read through
`type(self)`."""
import contextlib
import os

import numpy as np

from . import logit_edits as edit_np
from . import logprobs as lp_np
from . import penalties as pen_np
from . import stop_sequences as ss_np
from . import token_fsm as fsm_np
from .sampling import Table, params_bytes


# the entry points of the wide step: a library (or ABI stand-in) without them keeps B > 8 on the generic step
_WIDE_ENTRIES = ("pdn_decode_wide_supported", "pdn_decode_wide_blocks", "pdn_decode_wide_work_floats",
                 "pdn_decode_wide_gemm_f32", "pdn_decode_wide_pick_tick_rows_f32", "pdn_decode_wide_pick_tick_slots_f32",
                 "pdn_decode_wide_sample_tick_rows_f32", "pdn_decode_wide_sample_tick_slots_f32")
# ... and of the mixed step of chunked prefill (csrc/extend.hip), which runs on the wide product at any row count
_MIXED_ENTRIES = _WIDE_ENTRIES + ("pdn_decode_mixed_supported", "pdn_kv_append_rows_f32", "pdn_decode_extend_attention_f32")
# ... and of the speculative pass (csrc/speculative.hip), which runs the mixed step's layers
_SPEC_ENTRIES = _MIXED_ENTRIES + ("pdn_spec_draft_rows", "pdn_spec_verify_pick_tick_f32", "pdn_spec_verify_sample_tick_f32")
# the entry points of the penalties (csrc/penalty.hip): without them every path applies the statement of llm/penalties.py
_PEN_ENTRIES = ("pdn_penalty_chunks", "pdn_penalty_reset", "pdn_penalty_step_f32", "pdn_penalty_rows_f32")
# the entry points of the logit edits (csrc/logit_edit.hip, include/pdn_logitedit.h): without them every path applies the
# statement of llm/logit_edits.py
_EDIT_ENTRIES = ("pdne_logit_edit_chunks", "pdne_logit_edit_reset", "pdne_logit_edit_step_f32", "pdne_logit_edit_rows_f32")
# the entry points of the token FSM (csrc/token_fsm.hip, include/pdn_fsm.h): without them every path applies the statement of
# llm/token_fsm.py
_FSM_ENTRIES = ("pdnf_fsm_chunks", "pdnf_fsm_reset", "pdnf_fsm_step_f32", "pdnf_fsm_rows_f32")
# the entry points of the stop sequences (csrc/stop_seq.hip, include/pdn_stopseq.h): without them the plan refuses and every
# path stops its rows by the host matcher of llm/stop_sequences.py
_STOPSEQ_ENTRIES = ("pdnh_stop_reset", "pdnh_stop_step")
# the per-row sampled launches (include/pdn_persample.h): without them a run with a parameter table leaves the graph path and
# every draw applies the statement of llm/sampling.py row by row
_PERSAMPLE_ENTRIES = ("pdnq_sample_rows_f32", "pdnq_decode_sample_tick_rows_f32", "pdnq_decode_sample_tick_slots_f32",
                      "pdnq_decode_wide_sample_tick_rows_f32", "pdnq_decode_wide_sample_tick_slots_f32",
                      "pdnq_spec_verify_sample_tick_f32")
# ring slots of the log-probability records of a decode plan (csrc/logprobs.hip): more than the steps ever in flight
_LP_RING = 8


class DecodePlan:
    def _fast_path(self, dev):
        """Whether generation on device `dev` takes the HIP decode fast path: fast_decode on, a HIP device, inference
        mode, float32 weights and a head dimension the kernels' float4 loads take."""
        return bool(type(self).fast_decode and dev.is_hip and not self._train
                    and self.lm_head.weight.dtype == np.float32 and (self.embed_dim // self.n_heads) % 4 == 0)

    def _head_bias(self):
        """The address of the lm_head bias, or None for a head without one."""
        bias = getattr(self.lm_head, "bias", None)
        return bias.data._ptr if bias is not None else None

    def _stop_mask(self, stops):
        """The stop ids (int64 array) as the bitmask the ticks test: bit t of ceil(V / 32) int32 words."""
        mask = np.zeros(-(-self.vocab_size // 32), np.uint32)
        np.bitwise_or.at(mask, stops >> 5, np.uint32(1) << (stops & 31).astype(np.uint32))
        return mask.view(np.int32)

    def _decode_plan(self, B, sampling=False, ragged=False, serve=False, beam=0, n_stops=0, penalty=False, n_lp=None,
                     edit=False, per_row=False, fsm=False, stopseq=False):
        """Buffers and weight views of the graph-replayable decode step (csrc/decode.hip), or None when the
        model's shapes / layout are outside what those kernels take (then the generic launches below run).
        `sampling`: the step ends in the sample tick (csrc/sample.hip) instead of the greedy pick; its parameters live in
        the plan's `params` buffer, so new values never re-capture.
        `ragged` (generate_ragged): every row at its own position -- `pos` is (B,) int32 (-1: a stopped row), the
        *_rows_f32 entries run, the tick indexes the history by the device step counter `step` and stops rows whose
        token is set in the `stop` bitmask.
        `serve` (Llama.serve, with `ragged`): the step ends in the slot ticks -- `req` (B,) int32 holds the counter id of
        each row, `left` (B,) int32 the tokens it may still produce -- and the history is a ring of `ring` steps.
        `beam` (Llama.beam_search, with `ragged`): W beams per group and `n_stops` stop ids; the projection writes full
        logit rows and the tick is replaced by top-k -> select -> KV-cache reorder (csrc/beam.hip, buffers in `bm`).
        More than 8 rows (`wide_decode`): the wide step of csrc/decode_wide.hip, always in the per-row form (`rows`; a
        rectangular batch holds equal positions and a step counter equal to the position).
        `penalty` (generation with penalties, csrc/penalty.hip): the projection writes full logit rows, and
        pdn_penalty_step_f32 counts each row's fed token and penalises them before the tick; the rows' counts / prompt
        bits / prompt lengths live in the plan (`counts`, `seen`, `start`), the values in `pen_params`.  A greedy plan's
        `cand_v` / `cand_i` then hold the candidates of that kernel.  None when the library lacks the entries.
        `n_lp` (generation with logprobs=n, csrc/logprobs.hip): pdn_logprobs_tick_f32 after the tick reads the logit rows
        (which every plan writes) and the token the tick stored, and writes each row's record into a ring of `_LP_RING`
        slots of mapped host memory (`lp_box`, reached through the device pointer `lp_ptr`).
        `edit` (generation with allowed_token_ids / logit_bias / min_new_tokens, csrc/logit_edit.hip): the projection writes
        full logit rows, and pdne_logit_edit_step_f32 edits them before the tick (after the penalty kernel); the rows'
        allowed bits, bias tables and prompt lengths live in the plan (`edit_allow`, `edit_allow_on`, `edit_bias_ids`,
        `edit_bias_val`, `edit_bias_n`, `edit_start`), min_new_tokens in `edit_params`.  A greedy plan's `cand_v` / `cand_i`
        then hold the candidates of that kernel.  None when the library lacks the entries.
        `per_row` (a sampled run of generate_ragged / serve with a parameter table, llm/sampling.Table; with `ragged`):
        `params` holds a block per row, (B, 3) int64, and the step ends in the pdnq_ tick of include/pdn_persample.h, where
        row b is drawn with block b.  None when the library lacks the entries.
        `fsm` (generation with token_fsm, csrc/token_fsm.hip; False, or the (states, edges) capacity of the call's merged
        machines, llm/token_fsm.Machines.caps): the projection writes full logit rows, and pdnf_fsm_step_f32 advances each
        row's state by the token it is fed and masks its logits between the penalty kernel and the edit kernel; the tables
        live in the plan at that capacity (`fsm_off`, `fsm_tok`, `fsm_next`, `fsm_dflt`: a later call's machines of similar
        size are uploaded into the same arrays), the rows' state words, start states and prompt lengths in `fsm_state`,
        `fsm_start_state`, `fsm_start`.  A greedy plan's `cand_v` / `cand_i` then hold the candidates of the last of the
        three kernels.  None when the library lacks the entries.
        `stopseq` (generate_ragged / serve with stop_sequences, csrc/stop_seq.hip; False, or the (sets, sequences, tokens)
        capacity of the call's tables, llm/stop_sequences.StopSeqs.caps; with `ragged`): pdnh_stop_step is the last launch
        of a step, behind the tick and the logprobs tick -- it appends the token the tick stored to the row's tail ring
        and stops the row (pos = -1) when one of its sequences ends there; the tables live in the plan at that capacity
        (`ss_set_off`, `ss_seq_off`, `ss_toks`), the rows' set ids, prompt lengths and tails in `ss_set`, `ss_start`,
        `ss_tail`, min_new_tokens in `ss_min`.  None when the library lacks the entries."""
        from .. import hipnp as hp, _lib
        D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        st = getattr(self, "_decode_st", None)
        # a captured step (and the stacked weight views) hold the address of EVERY array the launches read: the key
        # covers them all -- rebinding `.data` of any parameter / cache re-plans -- and the switches that shape the plan
        ptrs = self._weight_ptrs()
        cache_len = self.layers[0].attention.cache_k.shape[1]
        wide = B > 8 and type(self).wide_decode and self._decode_wide_ok(B, cache_len)
        key = (B, hp._state["device"], int(type(self).fused_decode or 0), os.environ.get("PDN_DECODE_SPLITS", ""),
               cache_len, tuple(ptrs), bool(sampling), wide,   # (the addresses: no hash to collide)
               (int(beam), int(n_stops), bool(penalty)), bool(ragged), bool(serve)) + (() if n_lp is None else (int(n_lp),))
        key += ("edit",) if edit else ()
        key += ("per_row",) if per_row else ()
        key += ("fsm",) + tuple(int(c) for c in fsm) if fsm else ()
        key += ("stopseq",) + tuple(int(c) for c in stopseq) if stopseq else ()
        if st is not None and st["key"] == key:
            return st if st["ok"] else None
        if st is not None:
            for g in st.get("graphs", {}).values():
                g.destroy()
        ok = (B <= 8 and B * max(D, F) <= 16384 and D % 4 == 0 and F % 4 == 0 and V % 4 == 0 and (D // H) % 4 == 0
              and self.layers[0].attention.cache_k.shape[1] * 4 <= 60 * 1024 and D // H <= 256)
        if wide:
            # (the merge of the key-range partials happens in the output projection's load: at most 8 ranges)
            ok = int(os.environ.get("PDN_DECODE_SPLITS", "0") or 0) <= 8
        if penalty and not all(_lib.provides(n) for n in _PEN_ENTRIES):
            ok = False
        if edit and not all(_lib.provides(n) for n in _EDIT_ENTRIES):
            ok = False
        if per_row and not all(_lib.provides(n) for n in _PERSAMPLE_ENTRIES):
            ok = False
        if fsm and not all(_lib.provides(n) for n in _FSM_ENTRIES):
            ok = False
        if stopseq and not (ragged and all(_lib.provides(n) for n in _STOPSEQ_ENTRIES)):
            ok = False
        packs = []
        if ok:
            for layer in self.layers:
                a, f = layer.attention, layer.ffn
                qkv = hp.stacked_view([a.Q.weight.data, a.K.weight.data, a.V.weight.data])
                gu = hp.stacked_view([f.gate.weight.data, f.up.weight.data])
                mats = (a.O.weight.data, f.down.weight.data)
                if qkv is None or gu is None or not all(m.is_contiguous() for m in mats):    # (block strides may be < 0)
                    ok = False
                    break
                packs.append((qkv, gu))
            ok = ok and self.lm_head.weight.data.is_contiguous() and self.tok_embedding.weight.data.is_contiguous()
        st = {"B": B, "key": key, "ok": ok, "sampling": bool(sampling), "ragged": bool(ragged), "serve": bool(serve),
              "wide": wide, "rows": bool(ragged or wide), "beam": int(beam),
              "full": bool(sampling or beam or penalty or edit or fsm),
              "pen": bool(penalty), "lp_n": n_lp, "edit": bool(edit), "per_row": bool(per_row), "fsm": bool(fsm),
              "stopseq": bool(stopseq)}
        if ok:
            nblk = _lib.lib().query("pdn_decode_wide_blocks" if wide else "pdn_decode_gemv_blocks", V)
            # key ranges per head in the decode attention: one CU pulls ~11 B/clk, so long caches are cut up
            ns = int(os.environ.get("PDN_DECODE_SPLITS", "0")) or (1 if self.layers[0].attention.cache_k.shape[1] <= 256 else 4)
            st.update(packs=packs, graphs={}, nograph=False, host_pos=None, ns=ns,
                      ids=hp.zeros((B, 1), np.int64), pos=hp.zeros((1,), np.int32),
                      cand_v=hp.empty((B, nblk), np.float32), cand_i=hp.empty((B, nblk), np.int32),
                      # tokens by position: (*hist_ptr)[pos] is what the step at `pos` picked -- the array handed to
                      # the caller; a fresh history per generation (the pointer lives on the device, the graph holds
                      # only ITS address), so arrays returned earlier are never rewritten
                      hist_ptr=hp.zeros((1,), np.int64), hist=None,
                      # pdn_sample_params of the current generation (written before its first step; sampling plans only)
                      # (a plan with a parameter table: a block per row)
                      params=hp.zeros((B, 3) if per_row else (3,), np.int64) if sampling else None, params_val=None,
                      **{n: hp.empty((B, w), np.float32) for n, w in
                         (("x", D), ("qkv", 3 * D), ("att", ns * H * (4 + D // H)), ("gu", 2 * F), ("logits", V))})
            # three launches per layer (csrc/decode_layer.hip): the output / down projections leave per-head /
            # per-32-hidden-unit records that the next kernel's staging adds to the residual row
            J = _lib.lib().query("pdn_decode_mlp_slices", F)
            st["fused"] = bool(not wide and type(self).fused_decode and J and D <= 1024 and ns * H <= 256 and len(self.layers) > 0 and all(
                l.ffn.gate.weight.data.is_contiguous() and l.ffn.up.weight.data.is_contiguous() for l in self.layers))
            # two launches per layer (csrc/decode_block.hip): the q | k | v projection inside the attention kernel, one
            # more record per head for the new key
            st["block"] = bool(st["fused"] and int(type(self).fused_decode) >= 2 and
                               _lib.lib().query("pdn_decode_block_supported", D, H, D // H, ns))
            # (block path: the number of key ranges follows the position -- 256 cached keys per range, one captured
            #  step per count -- unless PDN_DECODE_SPLITS pins it)
            cache_len = self.layers[0].attention.cache_k.shape[1]
            st["ns_max"] = ns if os.environ.get("PDN_DECODE_SPLITS") else min(7, max(1, -(-(cache_len - 1) // 256)))
            if st["block"] and not _lib.lib().query("pdn_decode_block_supported", D, H, D // H, st["ns_max"]):
                st["ns_max"] = ns
            # a workgroup of the block kernel holds the scores of ceil(cache_len / ranges) positions in LDS whatever the
            # position: `ns_min` = the fewest ranges a cache of this length allows (long caches start above one range);
            # none up to ns_max -> the three-launch path
            st["ns_min"] = 1
            if st["block"]:
                fits = [n for n in range(1, st["ns_max"] + 1)
                        if 0 < _lib.lib().query("pdn_decode_block_lds_bytes", D, H, D // H, n, cache_len) <= 64 * 1024]
                if fits:
                    st["ns_min"] = fits[0]
                else:
                    st["block"] = False
            if st["fused"]:
                st.update(J=J, recs=hp.empty((B, (max(ns, st["ns_max"]) + 1) * H * (4 + D)), np.float32), dparts=hp.empty((B, J * D), np.float32),
                          xa=hp.empty((B, D), np.float32), xb=hp.empty((B, D), np.float32))
            if ragged or wide:
                st.update(pos=hp.zeros((B,), np.int32), step=hp.zeros((1,), np.int32),
                          stop=hp.zeros((-(-V // 32),), np.int32), run=None, host_step=None)
            if wide:
                # the wide ticks count their rows in at `arrive`; the split products keep partial tiles and arrival
                # counters in `work` (both zero between launches)
                work = max(_lib.lib().query("pdn_decode_wide_work_floats", B, k, n)
                           for k, n in ((D, 3 * D), (D, D), (F, D), (D, 2 * F), (D, V)))
                st.update(arrive=hp.zeros((1,), np.int32), work=hp.zeros((max(work, 4),), np.float32))
            if serve:
                st.update(req=hp.zeros((B,), np.int32), left=hp.zeros((B,), np.int32), ring=4, pending=0, issued=0)
            if beam:
                st["bm"] = self._beam_buffers(B, int(beam), int(n_stops), cache_len + 2)
            if penalty:
                # (B = 256, V = 32000: 33 MB of counts -- penalty plans only)
                st.update(counts=hp.zeros((B, V), np.int32), seen=hp.zeros((B, -(-V // 32)), np.int32),
                          start=hp.zeros((B,), np.int32), pen_params=hp.zeros((2,), np.int64), pen_val=None, pen_run=None)
                if not sampling:
                    nc = _lib.lib().query("pdn_penalty_chunks", V)
                    st.update(cand_v=hp.empty((B, nc), np.float32), cand_i=hp.empty((B, nc), np.int32))
            if edit:
                st.update(edit_allow=hp.zeros((B, -(-V // 32)), np.int32), edit_allow_on=hp.zeros((B,), np.int32),
                          edit_bias_ids=hp.zeros((B, edit_np.MAX_BIAS), np.int32),
                          edit_bias_val=hp.zeros((B, edit_np.MAX_BIAS), np.float32), edit_bias_n=hp.zeros((B,), np.int32),
                          edit_start=hp.zeros((B,), np.int32), edit_params=hp.zeros((2,), np.int64), edit_val=None,
                          edit_run=None)
                if not sampling:
                    nc = _lib.lib().query("pdne_logit_edit_chunks", V)
                    st.update(cand_v=hp.empty((B, nc), np.float32), cand_i=hp.empty((B, nc), np.int32))
            if fsm:
                S_cap, E_cap = (int(c) for c in fsm)
                st.update(fsm_off=hp.zeros((S_cap + 1,), np.int32), fsm_tok=hp.zeros((E_cap,), np.int32),
                          fsm_next=hp.zeros((E_cap,), np.int32), fsm_dflt=hp.zeros((S_cap,), np.int32),
                          fsm_state=hp.zeros((B,), np.int64), fsm_start_state=hp.zeros((B,), np.int32),
                          fsm_start=hp.zeros((B,), np.int32), fsm_caps=(S_cap, E_cap), fsm_val=None, fsm_run=None)
                if not sampling and not edit:
                    nc = _lib.lib().query("pdnf_fsm_chunks", V)
                    st.update(cand_v=hp.empty((B, nc), np.float32), cand_i=hp.empty((B, nc), np.int32))
            if stopseq:
                caps = tuple(int(c) for c in stopseq)
                st.update(ss_set_off=hp.zeros((caps[0] + 1,), np.int32), ss_seq_off=hp.zeros((caps[1] + 1,), np.int32),
                          ss_toks=hp.zeros((caps[2],), np.int32), ss_set=hp.asarray(np.full(B, -1, np.int32)),
                          ss_start=hp.zeros((B,), np.int32), ss_tail=hp.asarray(np.full((B, ss_np.MAX_LEN), -1, np.int32)),
                          ss_min=hp.zeros((1,), np.int32), ss_caps=caps, ss_val=None, ss_run=None)
            if n_lp is not None:
                st.update(lp_ptr=hp.zeros((1,), np.int64), lp_box=None, lp_work=hp.zeros(
                    (_lib.lib().query("pdn_logprobs_work_bytes", B, V, n_lp) // 8 + 2,), np.int64))
            self._decode_ws = {"logits": st["logits"], "x": st["x"]}
        self._decode_st = st
        return st if ok else None

    def _weight_ptrs(self):
        """The address of every array a captured step reads (parameters, caches, RoPE tables): part of a plan's key."""
        ptrs = [self.lm_head.weight.data._ptr, self.tok_embedding.weight.data._ptr, self.norm.weight.data._ptr,
                self.freqs_cos.data._ptr, self.freqs_sin.data._ptr]
        bias = getattr(self.lm_head, "bias", None)
        ptrs.append(bias.data._ptr if bias is not None else 0)
        for layer in self.layers:
            a, f = layer.attention, layer.ffn
            ptrs += [t.data._ptr for t in (a.Q.weight, a.K.weight, a.V.weight, a.O.weight, a.cache_k, a.cache_v,
                                            f.gate.weight, f.up.weight, f.down.weight, layer.input_norm.weight,
                                            layer.post_attn_norm.weight)]
        return ptrs

    def _decode_wide_ok(self, B, cache_len):
        """Whether the library provides the wide step and takes this model with B rows; asked once per (library, B,
        cache length), not at every step."""
        from .. import _lib
        L, D, H, F, V = _lib.lib(), self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        memo = getattr(self, "_wide_memo", None)
        if memo is not None and memo[0] is L and memo[1] == (B, D, H, F, V, cache_len):
            return memo[2]
        ok = bool(all(_lib.provides(n) for n in _WIDE_ENTRIES)
                  and L.query("pdn_decode_wide_supported", B, D, H, D // H, F, V, cache_len))
        self._wide_memo = (L, (B, D, H, F, V, cache_len), ok)
        return ok

    def _decode_ns(self, st, pos):
        """Key ranges per head for the step at position `pos`."""
        if not st.get("block"):
            return st["ns"]
        if os.environ.get("PDN_DECODE_SPLITS"):
            return max(st["ns"], st.get("ns_min", 1))
        return min(st["ns_max"], max(st.get("ns_min", 1), -(-pos // 256)))

    def _decode_launches(self, st, ns=None):
        """The launches of one decode step (2 per layer + 2; 3 or 5 per layer at lower `fused_decode` levels); every argument is fixed for the lifetime of `st` (the position
        and the token ids are read from device memory), so the sequence can be captured once and replayed."""
        from .. import hipnp as hp, _lib
        L, s = _lib.lib(), hp.stream()
        D, H, F, V, B = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size, st["B"]
        hd = D // H
        x, qkv, att, gu, logits = (st[n]._ptr for n in ("x", "qkv", "att", "gu", "logits"))
        pos = st["pos"]._ptr
        # (ragged plans: the same launches through the entries with a position per row)
        rows = "rows_" if st["rows"] else ""
        # (x = embedding rows of the current ids: left there by the previous step's pick kernel, or by
        #  `_decode_gather` when the ids came from outside)
        emb = self.tok_embedding.weight.data
        cos, sin = self.freqs_cos.data._ptr, self.freqs_sin.data._ptr
        head, bias = self.lm_head, self._head_bias()
        if st["wide"]:
            self._decode_launches_wide(st, s)
            return
        if st["fused"]:
            J, ns = st["J"], (st["ns"] if ns is None else ns)
            recs, dparts, xa, xb = (st[n]._ptr for n in ("recs", "dparts", "xa", "xb"))
            rrs = ns * H * (4 + D)
            for li, (layer, (wqkv, _)) in enumerate(zip(self.layers, st["packs"])):
                a, f = layer.attention, layer.ffn
                ck, cv = a.cache_k.data, a.cache_v.data
                nrm = layer.input_norm
                if st["block"]:
                    # x = previous block's h + its feed-forward records (-> xa); q | k | v, RoPE, cache append, attention
                    # and each head's rows of Wo in one launch: records of ns key ranges + the new key
                    L.call(f"pdn_decode_block_{rows}f32", x if li == 0 else xb, D, None if li == 0 else dparts, 0 if li == 0 else J,
                           J * D, xa, D, nrm.weight.data._ptr, nrm.eps, wqkv._ptr, D, wqkv._strides[0], cos, sin, ck._ptr,
                           cv._ptr, ck._strides[0], pos, ck.shape[1], a.O.weight.data._ptr, D, recs, B, H, hd, ns, s)
                    nrm = layer.post_attn_norm
                    L.call("pdn_decode_mlp_f32", xa, D, recs, (ns + 1) * H * (4 + D), ns + 1, H, xb, D,
                           nrm.weight.data._ptr, nrm.eps, f.gate.weight.data._ptr, f.up.weight.data._ptr, F,
                           f.down.weight.data._ptr, D, dparts, J * D, B, D, F, s)
                    continue
                # [q | k | v] = RMSNorm(x) @ [Wq | Wk | Wv]; x = previous block's h + its feed-forward records
                if li == 0:
                    L.call("pdn_decode_gemv_f32", x, D, nrm.weight.data._ptr, nrm.eps, wqkv._ptr, D, D, wqkv._strides[0],
                           None, None, 0, qkv, 3 * D, B, D, 3 * D, 0, 0, 0, None, None, s)
                else:
                    L.call("pdn_decode_gemv_sum_f32", xb, D, dparts, J, J * D, xa, D, nrm.weight.data._ptr, nrm.eps,
                           wqkv._ptr, D, D, wqkv._strides[0], None, qkv, 3 * D, B, D, 3 * D, None, None, s)
                # RoPE, cache append, attention over [0, pos], each head times its rows of Wo -> records
                L.call(f"pdn_decode_attention_oproj_{rows}f32", qkv, 3 * D, cos, sin, ck._ptr, cv._ptr, a.O.weight.data._ptr, D,
                       recs, B, H, hd, ns, ck._strides[0], pos, ck.shape[1], s)
                # h = x + merged records (-> xb); 32 hidden units per workgroup: gate | up, SwiGLU, their rows of Wdown
                nrm = layer.post_attn_norm
                L.call("pdn_decode_mlp_f32", x if li == 0 else xa, D, recs, rrs, ns, H, xb, D, nrm.weight.data._ptr,
                       nrm.eps, f.gate.weight.data._ptr, f.up.weight.data._ptr, F, f.down.weight.data._ptr, D, dparts,
                       J * D, B, D, F, s)
            cv, ci = (None, None) if st["full"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
            L.call("pdn_decode_gemv_sum_f32", xb, D, dparts, J, J * D, None, 0, self.norm.weight.data._ptr, self.norm.eps,
                   head.weight.data._ptr, V, V, 0, bias, logits, V, B, D, V, cv, ci, s)
            self._pen_step(st, s)
            self._fsm_step(st, s)
            self._edit_step(st, s)
            self._decode_tick(st, s)
            self._lp_tick(st, s)
            self._stop_step(st, s)
            return
        for layer, (wqkv, wgu) in zip(self.layers, st["packs"]):
            a, f = layer.attention, layer.ffn
            ck, cv = a.cache_k.data, a.cache_v.data
            cbs = ck._strides[0]
            # h = RMSNorm(x); [q | k | v] = h @ [Wq | Wk | Wv]
            L.call("pdn_decode_gemv_f32", x, D, layer.input_norm.weight.data._ptr, layer.input_norm.eps, wqkv._ptr, D, D,
                   wqkv._strides[0], None, None, 0, qkv, 3 * D, B, D, 3 * D, 0, 0, 0, None, None, s)
            # RoPE of q / k, cache append, attention over positions [0, pos]
            L.call(f"pdn_decode_attention_{rows}f32", qkv, 3 * D, cos, sin, ck._ptr, cv._ptr, att, B, H, hd, st["ns"], cbs, pos,
                   ck.shape[1], s)
            wo, wd = a.O.weight.data, f.down.weight.data
            # x += merge(att partials) @ Wo: the key-range partials are merged while the row is staged
            L.call("pdn_decode_gemv_f32", att, st["att"].shape[1], None, 0.0, wo._ptr, D, D, 0, None, x, D, x, D, B, D, D,
                   2, st["ns"], hd, None, None, s)
            L.call("pdn_decode_gemv_f32", x, D, layer.post_attn_norm.weight.data._ptr, layer.post_attn_norm.eps, wgu._ptr,
                   F, F, wgu._strides[0], None, None, 0, gu, 2 * F, B, D, 2 * F, 0, 0, 0, None, None, s)
            # x += (silu(gate) * up) @ Wdown: SwiGLU in the loads
            L.call("pdn_decode_gemv_f32", gu, 2 * F, None, 0.0, wd._ptr, D, D, 0, None, x, D, x, D, B, F, D, 1, 0, 0,
                   None, None, s)
        # vocabulary projection; every workgroup also leaves the first maximum of its columns, the pick kernel
        # finishes the argmax over those candidates (model.py:262-268) and advances the position
        cv, ci = (None, None) if st["full"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        L.call("pdn_decode_gemv_f32", x, D, self.norm.weight.data._ptr, self.norm.eps, head.weight.data._ptr, V, V, 0,
               bias, None, 0, logits, V, B, D, V, 0, 0, 0, cv, ci, s)
        self._pen_step(st, s)
        self._fsm_step(st, s)
        self._edit_step(st, s)
        self._decode_tick(st, s)
        self._lp_tick(st, s)
        self._stop_step(st, s)

    def _decode_launches_wide(self, st, s):
        """The wide step (9 .. 256 rows, csrc/decode_wide.hip): 5 launches per layer -- q | k | v with RMSNorm in the load,
        the per-row attention, x += merge(partials) @ Wo, gate | up with RMSNorm in the load, x += SwiGLU(gate | up) @
        Wdown -- then the vocabulary projection (+ candidates of the greedy pick) and the wide tick."""
        from .. import _lib
        L = _lib.lib()
        D, H, F, V, B = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size, st["B"]
        hd, ns = D // H, st["ns"]
        x, qkv, att, gu, logits, pos, work = (st[n]._ptr for n in ("x", "qkv", "att", "gu", "logits", "pos", "work"))
        cos, sin = self.freqs_cos.data._ptr, self.freqs_sin.data._ptr
        for layer, (wqkv, wgu) in zip(self.layers, st["packs"]):
            a, f = layer.attention, layer.ffn
            ck, cv = a.cache_k.data, a.cache_v.data
            nrm = layer.input_norm
            L.call("pdn_decode_wide_gemm_f32", x, D, 1, nrm.weight.data._ptr, nrm.eps, 0, 0, wqkv._ptr, D, D,
                   wqkv._strides[0], None, qkv, 3 * D, 0, None, None, pos, B, D, 3 * D, work, s)
            L.call("pdn_decode_attention_rows_f32", qkv, 3 * D, cos, sin, ck._ptr, cv._ptr, att, B, H, hd, ns,
                   ck._strides[0], pos, ck.shape[1], s)
            L.call("pdn_decode_wide_gemm_f32", att, st["att"].shape[1], 3, None, 0.0, ns, hd, a.O.weight.data._ptr, D, D,
                   0, None, x, D, 1, None, None, pos, B, D, D, work, s)
            nrm = layer.post_attn_norm
            L.call("pdn_decode_wide_gemm_f32", x, D, 1, nrm.weight.data._ptr, nrm.eps, 0, 0, wgu._ptr, F, F,
                   wgu._strides[0], None, gu, 2 * F, 0, None, None, pos, B, D, 2 * F, work, s)
            L.call("pdn_decode_wide_gemm_f32", gu, 2 * F, 2, None, 0.0, 0, 0, f.down.weight.data._ptr, D, D, 0, None,
                   x, D, 1, None, None, pos, B, F, D, work, s)
        head, bias = self.lm_head, self._head_bias()
        cv, ci = (None, None) if st["full"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        L.call("pdn_decode_wide_gemm_f32", x, D, 1, self.norm.weight.data._ptr, self.norm.eps, 0, 0, head.weight.data._ptr,
               V, V, 0, bias, logits, V, 0 if st["full"] else 2, cv, ci, pos, B, D, V, work, s)
        self._pen_step(st, s)
        self._fsm_step(st, s)
        self._edit_step(st, s)
        self._decode_tick(st, s)
        self._lp_tick(st, s)
        self._stop_step(st, s)

    def _lp_tick(self, st, s):
        """Plans with logprobs: after the tick, each row's record (csrc/logprobs.hip) of the step the tick just finished
        -- the counter it advanced, the token it stored in the history -- into the plan's record ring."""
        if st.get("lp_n") is None:
            return
        from .. import _lib
        V, B = self.vocab_size, st["B"]
        cnt = st["step"] if st["rows"] else st["pos"]
        _lib.lib().call("pdn_logprobs_tick_f32", st["logits"]._ptr, V, B, V, st["lp_n"], st["hist_ptr"]._ptr,
                        st["ring"] if st["serve"] else 0, cnt._ptr, st["lp_ptr"]._ptr, _LP_RING, st["lp_work"]._ptr, s)

    def _hist_begin(self, st, hist):
        """A new run stores its tokens into the Mailbox `hist`: the history pointer goes there, and a plan with logprobs
        gets a fresh record ring (both stream ordered)."""
        from .. import hipnp as hp
        st["hist_ptr"][...] = np.int64(hist._ptr)
        if st.get("lp_n") is not None:
            st["lp_box"] = hp.Mailbox(_LP_RING, (st["B"], lp_np.record_words(st["lp_n"])), unset=lp_np.UNSET)
            st["lp_ptr"][...] = np.int64(st["lp_box"]._ptr)

    def _run_values(self, st, sampling, pen=None, edit=None, fsm=None, stopseq=None, lens=None):
        """The values of a run, uploaded when they differ from those in the plan (stream ordered: earlier steps read the
        old ones): the sampling parameters (a llm/sampling.Table: row b takes request b's block; a served plan's rows take
        theirs at admission, `_params_rows`), and for a run with penalties (`pen`: its llm/penalties.Rows) every row's
        prompt with zero counts; for a run with logit edits (`edit`: its llm/logit_edits.Rows) every row's request; for a
        run with machines (`fsm`: its llm/token_fsm.Rows) the tables and every row's start state; for a run with stop
        sequences (`stopseq`: its llm/stop_sequences.Rows, fed the rows' first tokens) the tables and every row's set,
        prompt length and first token (`lens`: the prompt lengths) -- and, for a run that comes back mid-stream, the rings of
        its matcher."""
        if st["params_val"] != sampling:
            if isinstance(sampling, Table):
                if not st.get("serve"):
                    self._params_rows(st, sampling, np.arange(st["B"]))
            elif sampling is not None:
                st["params"][...] = params_bytes(*sampling)
            st["params_val"] = sampling
        if pen is not None and st["pen_run"] is not pen:
            self._pen_reset(st, np.arange(st["B"]), pen.prompts, pen.values)
            st["pen_run"] = pen
        if edit is not None and st["edit_run"] is not edit:
            self._edit_reset(st, np.arange(st["B"]), edit.req, edit.start, edit.spec)
            st["edit_run"] = edit
        if fsm is not None and st["fsm_run"] is not fsm:
            self._fsm_reset(st, np.arange(st["B"]), fsm.req, fsm.start, fsm.spec)
            st["fsm_run"] = fsm
        if stopseq is not None and st["ss_run"] is not stopseq:
            self._stop_reset(st, np.arange(st["B"]), stopseq.set, lens, stopseq.first, stopseq.spec)
            if (stopseq.count > 1).any():
                # (a run that comes back to the plan mid-stream, after another generation used it: the rings as the
                #  host matcher holds them, slot for slot the device's)
                st["ss_tail"][...] = stopseq.tail
            st["ss_run"] = stopseq

    @staticmethod
    def _params_rows(st, table, reqs):
        """The rows of a plan with a parameter table take the blocks of requests `reqs` (B,) (< 0: a free row, whose block
        is never read); stream ordered, so only while no step is queued that may still read the old ones."""
        st["params"][...] = table.blocks(reqs)

    def _lp_read(self, st, i):
        """The records of step i (a poll of its ring slot, then marked unwritten again) as Logprobs."""
        box, k = st["lp_box"], i % _LP_RING
        rec = np.array(box.slot(k).get()).reshape(st["B"], -1)
        box.host[k] = box.unset
        return lp_np.from_records(rec, st["lp_n"])

    def _pen_step(self, st, s):
        """Penalty plans: between the vocabulary projection and the tick, each live row counts the token it is fed and its
        logits are penalised in place (greedy plans: with the candidates the tick reduces, csrc/penalty.hip)."""
        if not st["pen"]:
            return
        from .. import _lib
        V, B = self.vocab_size, st["B"]
        # (the candidates: of the FSM or the edit kernel when one of them runs behind this one)
        cv, ci = (None, None) if st["sampling"] or st["edit"] or st["fsm"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        _lib.lib().call("pdn_penalty_step_f32", st["logits"]._ptr, V, B, V, st["pen_params"]._ptr, st["counts"]._ptr,
                        st["seen"]._ptr, st["start"]._ptr, st["ids"]._ptr, st["pos"]._ptr, int(st["rows"]), cv, ci, s)

    def _fsm_step(self, st, s):
        """FSM plans: between the penalty kernel (or the vocabulary projection) and the edit kernel (or the tick), each
        live row's state is advanced by the token it is fed and its logits are masked in place (greedy plans without
        edits: with the candidates the tick reduces, csrc/token_fsm.hip)."""
        if not st["fsm"]:
            return
        from .. import _lib
        V, B = self.vocab_size, st["B"]
        cv, ci = (None, None) if st["sampling"] or st["edit"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        S_cap, E_cap = st["fsm_caps"]
        _lib.lib().call("pdnf_fsm_step_f32", st["logits"]._ptr, V, B, V, st["fsm_off"]._ptr, st["fsm_tok"]._ptr,
                        st["fsm_next"]._ptr, st["fsm_dflt"]._ptr, S_cap, E_cap, st["fsm_state"]._ptr,
                        st["fsm_start_state"]._ptr, st["fsm_start"]._ptr, st["ids"]._ptr, st["pos"]._ptr, int(st["rows"]),
                        cv, ci, s)

    def _fsm_reset(self, st, rows, reqs, lens, spec):
        """Rows `rows` of an FSM plan take requests `reqs` of `spec` (llm/token_fsm.Machines) with prompt lengths `lens`
        (start states, prompt lengths, state words; one launch, stream ordered after every step queued before), and the
        plan's tables become the call's (stream ordered too)."""
        from .. import hipnp as hp, _lib
        if st["fsm_val"] is not spec:
            for name, a in zip(("fsm_off", "fsm_tok", "fsm_next", "fsm_dflt"), fsm_np.padded(spec.tables, *st["fsm_caps"])):
                st[name][...] = a
            st["fsm_val"] = spec
        rows = np.asarray(rows, np.int32).reshape(-1)
        if not rows.size:
            return
        # (device copies held until the call has been issued; the allocator orders their reuse on the stream)
        d_rows, d_state = hp.asarray(rows), hp.asarray(spec.start_states(reqs))
        d_len = hp.asarray(np.asarray(lens, np.int32).reshape(-1))
        _lib.lib().call("pdnf_fsm_reset", st["fsm_state"]._ptr, st["fsm_start_state"]._ptr, st["fsm_start"]._ptr, st["B"],
                        d_rows._ptr, int(rows.size), d_state._ptr, d_len._ptr, hp.stream())

    def _stop_step(self, st, s):
        """Plans with stop sequences: the last launch of a step, behind the tick (and the logprobs tick) -- each row the
        tick left running appends the token it stored to its tail ring and stops (pos = -1) when one of its sequences
        ends there (csrc/stop_seq.hip)."""
        if not st["stopseq"]:
            return
        from .. import _lib
        _lib.lib().call("pdnh_stop_step", st["ids"]._ptr, st["pos"]._ptr, st["B"], st["ss_set_off"]._ptr,
                        st["ss_seq_off"]._ptr, st["ss_toks"]._ptr, *st["ss_caps"], st["ss_set"]._ptr, st["ss_start"]._ptr,
                        st["ss_tail"]._ptr, st["ss_min"]._ptr, s)

    def _stop_reset(self, st, rows, sets, lens, first, spec):
        """Rows `rows` of a plan with stop sequences take the set ids `sets` of `spec` (llm/stop_sequences.StopSeqs) with
        prompt lengths `lens`, a cleared tail and their first tokens `first` (-1, or None for all: it will come out of a
        replayed step); one launch, stream ordered after every step queued before.  The plan's tables and min_new_tokens
        become the call's (stream ordered too)."""
        from .. import hipnp as hp, _lib
        if st["ss_val"] is not spec:
            for name, a in zip(("ss_set_off", "ss_seq_off", "ss_toks"), ss_np.padded(spec.tables, st["ss_caps"])):
                st[name][...] = a
            st["ss_min"][...] = np.int32(spec.m)
            st["ss_val"] = spec
        rows = np.asarray(rows, np.int32).reshape(-1)
        if not rows.size:
            return
        first = np.full(rows.size, -1, np.int32) if first is None else np.asarray(first, np.int32).reshape(-1)
        # (device copies held until the call has been issued; the allocator orders their reuse on the stream)
        d_rows, d_set, d_first = hp.asarray(rows), hp.asarray(np.asarray(sets, np.int32).reshape(-1)), hp.asarray(first)
        d_len = hp.asarray(np.asarray(lens, np.int32).reshape(-1))
        _lib.lib().call("pdnh_stop_reset", st["ss_set"]._ptr, st["ss_start"]._ptr, st["ss_tail"]._ptr, st["B"],
                        d_rows._ptr, int(rows.size), d_set._ptr, d_len._ptr, d_first._ptr, hp.stream())

    def _edit_step(self, st, s):
        """Edit plans: between the vocabulary projection (or the penalty kernel) and the tick, each live row's logits are
        edited in place for its request (greedy plans: with the candidates the tick reduces, csrc/logit_edit.hip).  The
        stop ids of min_new_tokens are the tick's own bitmask (the rectangular `generate` has neither)."""
        if not st["edit"]:
            return
        from .. import _lib
        V, B = self.vocab_size, st["B"]
        cv, ci = (None, None) if st["sampling"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        stop = st["stop"]._ptr if st["ragged"] else None
        _lib.lib().call("pdne_logit_edit_step_f32", st["logits"]._ptr, V, B, V, st["edit_params"]._ptr,
                        st["edit_allow"]._ptr, st["edit_allow_on"]._ptr, st["edit_bias_ids"]._ptr, st["edit_bias_val"]._ptr,
                        st["edit_bias_n"]._ptr, st["edit_start"]._ptr, st["pos"]._ptr, int(st["rows"]), stop, cv, ci, s)

    def _edit_reset(self, st, rows, reqs, lens, spec):
        """Rows `rows` of an edit plan take requests `reqs` of `spec` (llm/logit_edits.Edits) with prompt lengths `lens`
        (allowed bits, bias tables, prompt lengths; one launch, stream ordered after every step queued before), and the
        plan's min_new_tokens becomes the call's (stream ordered too)."""
        from .. import hipnp as hp, _lib
        if st["edit_val"] != spec.m:
            st["edit_params"][...] = edit_np.params_bytes(spec.m)
            st["edit_val"] = spec.m
        rows = np.asarray(rows, np.int32).reshape(-1)
        if not rows.size:
            return
        # (device copies held until the call has been issued; the allocator orders their reuse on the stream)
        src = [None if a is None else hp.asarray(a) for a in spec.packed(reqs)]
        d_rows, d_len = hp.asarray(rows), hp.asarray(np.asarray(lens, np.int32).reshape(-1))
        _lib.lib().call("pdne_logit_edit_reset", st["edit_allow"]._ptr, st["edit_allow_on"]._ptr, st["edit_bias_ids"]._ptr,
                        st["edit_bias_val"]._ptr, st["edit_bias_n"]._ptr, st["edit_start"]._ptr, st["B"], self.vocab_size,
                        d_rows._ptr, int(rows.size), *(None if a is None else a._ptr for a in src), d_len._ptr,
                        hp.stream())

    def _pen_reset(self, st, rows, prompts, penalty):
        """Rows `rows` of a penalty plan take `prompts` (zero counts, prompt bits, prompt lengths; stream ordered after
        every step queued before), and the plan's values become `penalty` (stream ordered too)."""
        from .. import hipnp as hp, _lib
        if st["pen_val"] != penalty:
            st["pen_params"][...] = pen_np.params_bytes(*penalty)
            st["pen_val"] = penalty
        rows = np.asarray(rows, np.int32).reshape(-1)
        if not rows.size:
            return
        ids, off = pen_np.packed(prompts)
        # (device copies held until the call has been issued; the allocator orders their reuse on the stream)
        d_rows, d_ids, d_off = hp.asarray(rows), hp.asarray(ids) if ids.size else None, hp.asarray(off)
        _lib.lib().call("pdn_penalty_reset", st["counts"]._ptr, st["seen"]._ptr, st["start"]._ptr, st["B"],
                        self.vocab_size, d_rows._ptr, int(rows.size), d_ids._ptr if ids.size else None, d_off._ptr,
                        hp.stream())

    def _decode_tick(self, st, s, mixed=None):
        """The last launch of a step: the greedy pick over the projection's candidates, or (sampling plans) the sample
        tick over the full logit rows with counter (*pos, b); either stores the token and its embedding row, *pos += 1.
        The entry is pdn_decode[_wide]_{pick|sample}_tick[_rows|_slots]_f32 and its arguments are four groups: the source
        (logit rows + parameters, or candidates), the counters (the position(s); per-row plans: the step; wide: the
        rows' arrival count -- the last row to finish advances the step, csrc/decode_wide.hip), the slot state (served
        plans: counter id and token budget per row, the history ring; per-row plans: the stop bitmask) and the output.
        `mixed` (the mixed step's buffers): always the wide slot tick, on its own arrival counter and -- unless the
        penalty, the FSM or the edit kernel left the plan's -- its own candidates."""
        from .. import _lib
        emb, V, B = self.tok_embedding.weight.data, self.vocab_size, st["B"]
        if st["beam"]:
            self._beam_launches(st["bm"], st["logits"]._ptr, V, st["pos"]._ptr, st["step"]._ptr, st["ids"]._ptr,
                                st["x"]._ptr, first=False)
            return
        wide = st["wide"] or mixed is not None
        if st["sampling"]:
            src = (st["logits"]._ptr, V, B, V, st["params"]._ptr)
        else:
            c = st if mixed is None or st["pen"] or st["edit"] or st["fsm"] else mixed
            src = (c["cand_v"]._ptr, c["cand_i"]._ptr, B, c["cand_v"].shape[1])
        cnt = (st["pos"]._ptr,) + ((st["step"]._ptr,) if st["rows"] else ())
        if wide:
            cnt += ((st if mixed is None else mixed)["arrive"]._ptr,)
        slot = (st["req"]._ptr, st["left"]._ptr, st["ring"]) if st["serve"] else ()
        if st["rows"]:
            slot += (st["stop"]._ptr,)
        name = "pdn%s_decode%s_%s_tick%s_f32" % ("q" if st["per_row"] else "", "_wide" if wide else "",
                                                 "sample" if st["sampling"] else "pick",
                                                 "_slots" if st["serve"] else "_rows" if st["rows"] else "")
        _lib.lib().call(name, *src, st["ids"]._ptr, *cnt, *slot, st["hist_ptr"]._ptr, emb._ptr, emb._strides[0],
                        self.embed_dim, st["x"]._ptr, s)

    def _decode_gather(self, st):
        """x = tok_embedding[ids] for ids that did not come out of the previous step's pick kernel."""
        from .. import hipnp as hp, _lib
        emb = self.tok_embedding.weight.data
        _lib.lib().call("pdn_embedding_gather_f32", emb._ptr, self.vocab_size, self.embed_dim, emb._strides[0],
                        st["ids"]._ptr, st["B"], st["x"]._ptr, hp.err_flag_ptr(), hp.stream())

    def _issue(self, st, gkey, launches, keep=None, redirect=None, around=None, gather=True, graphs=None, capture=True):
        """Issue one step of plan `st`: replay its graph `graphs[gkey]` (`graphs`: `st["graphs"]` by default), captured
        first when there is none; or call `launches` -- the zero-argument callable that issues the step launch by launch
        -- when the plan is `nograph`, graph_decode is off or the caller rules a capture out (`capture`).  Returns
        whether a step was issued.
        `keep` = None: a step queued ahead.  It never captures, and while its graph is missing nothing is issued (False):
        the next real issue captures it.
        Otherwise a capture may happen.  hipnp.Graph runs the step twice for real (pool warm-up + first replay): those
        runs write the KV cache slots of the next two steps with exactly what the real steps will write there, and they
        advance ids, positions and counters.  `keep` maps the plan arrays to put back afterwards to their values: a host
        value, or None for a device copy taken before the capture.  A penalty plan's `counts` are always kept (the runs
        count their fed tokens too), an FSM plan's state words (the runs advance them) and the tails of a plan with stop
        sequences (the runs append to them and may stop rows: `pos` is kept by every caller).
        `redirect` = (name, mailbox[, slots]): the runs' tick stores its tokens through the device pointer st[name],
        which points at a SCRATCH twin of `mailbox` meanwhile, so that the real one's slots stay "not written" until the
        real steps store there (a later step with other ids would otherwise read the capture's token as its own).  The
        record ring of a plan with logprobs is treated the same way.  The scratch is built in this branch only.
        `around`: a context manager entered once the state is saved and left when the runs are done (the beam plan).
        `gather`: x = the embedding rows of the restored ids.
        PDN_EUNSUPPORTED from the capture (no graph support: the emulated ABI) turns the plan `nograph` -- plain launches
        from then on; anything else is a bug."""
        from .. import hipnp as hp, _lib
        graphs = st["graphs"] if graphs is None else graphs
        g = False if st["nograph"] else graphs.get(gkey)
        if g is None and keep is None:
            return False
        if g is None and capture and type(self).graph_decode:
            if st.get("pen"):
                keep = dict(keep, counts=None)
            if st.get("fsm"):
                keep = dict(keep, fsm_state=None)
            if st.get("stopseq"):
                keep = dict(keep, ss_tail=None)
            saved = {n: st[n].copy() if v is None else v for n, v in keep.items()}
            moved = [redirect] if redirect else []
            if st.get("lp_n") is not None:
                moved.append(("lp_ptr", st["lp_box"]))
            held = []                                            # (the scratch lives until the capture's runs are done)
            for name, box, *n in moved:
                held.append(hp.Mailbox(n[0] if n else box.n, box.shape, unset=box.unset))
                st[name][...] = np.int64(held[-1]._ptr)
            with around() if around else contextlib.nullcontext():
                try:
                    g = hp.Graph()
                    g.capture(launches)
                    graphs[gkey] = g
                except _lib.HipLibraryError as e:
                    if e.code != -2:
                        raise
                    st["nograph"], g = True, False
                hp.synchronize()
            for name, box, *_ in moved:
                st[name][...] = np.int64(box._ptr)
            for n, v in saved.items():
                st[n][...] = v
            if gather:
                self._decode_gather(st)
        if g:
            g.replay()
        else:
            launches()
        return True

    def _issue_step(self, st, top, keep=None, **how):
        """`_issue` for the plan's own step (`_decode_launches`) with its furthest row at position `top`: the range count
        of that position keys the graph."""
        ns = self._decode_ns(st, top)
        return self._issue(st, (ns, "beam" if st["beam"] else st["sampling"]), lambda: self._decode_launches(st, ns),
                           keep, **how)
