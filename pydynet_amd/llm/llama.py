"""6-layer Llama3 -- the north-star workload (llm/llama/model.py of the reference), restated
on this package's fused nodes.

Same constructor signature, same registered parameter names (`layers.{i}.attention.Q.weight`,
`layers.{i}.ffn.gate.weight`, `lm_head.bias`, ...), same construction order (so a seeded NumPy
RNG yields the reference's initial weights), same `forward_logits / finetune_step / forward /
generate` entry points.  What differs is the number of tape nodes per block: 62 in the
reference, 8 here on the training path (rms_norm, qkv_attention [3 projections + RoPE + causal
attention], linear+residual, rms_norm, 2x linear, swiglu, linear+residual), each a handful of HIP
kernels / GEMMs per direction; the separate linear / rope / attention nodes remain for shapes the
fused attention kernels do not cover and for the KV-cache path, whose per-token step bypasses the
tape altogether (`_decode_step_hip`).
"""
import math
import os

import numpy as np

from .. import nn
from ..autograd import is_grad_enable
from ..core import Tensor, fused
from ..special import zeros
from . import beam as beam_np
from . import chunked
from . import logprobs as lp_np
from . import penalties as pen_np
from . import prefix as prefix_np
from . import speculative as spec_np
from .sampling import (check_args as check_sampling_args, params_bytes, params_buffer, sample_next,
                       sample_next_rows)


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
# ring slots of the log-probability records of a decode plan (csrc/logprobs.hip): more than the steps ever in flight
_LP_RING = 8


def compute_cos_sin_cache(head_dim: int, max_seq_len: int, base: int = 10000, dtype=None):
    """cos/sin(outer(arange(max_seq_len), base^(-2i/head_dim))) -> two (max_seq_len, head_dim/2) tensors."""
    inv_freq = 1.0 / (base ** (np.arange(0, head_dim, 2)[: head_dim // 2] / head_dim))
    freqs = np.outer(np.arange(max_seq_len), inv_freq).astype(dtype)
    return Tensor(np.cos(freqs)), Tensor(np.sin(freqs))


def apply_rotary_emb(xq, xk, freqs_cos, freqs_sin):
    """Rotate interleaved pairs (x[2i], x[2i+1]) of q and k by the position angle: one fused node each."""
    return fused.rope(xq, freqs_cos, freqs_sin), fused.rope(xk, freqs_cos, freqs_sin)


class FeedForward(nn.Module):
    def __init__(self, dim, up_dim, dtype=None):
        super().__init__()
        self.dim, self.up_dim = dim, up_dim
        self.up = nn.Linear(dim, up_dim, bias=False, dtype=dtype)
        self.gate = nn.Linear(dim, up_dim, bias=False, dtype=dtype)
        self.down = nn.Linear(up_dim, dim, bias=False, dtype=dtype)

    def move(self, device):
        super().move(device)
        if device.is_hip:
            self._pack_gate_up()
        return self

    def _pack_gate_up(self):
        """Re-home the gate / up weights in one (2, dim, ffn) buffer: each stays a contiguous Parameter,
        and being equally spaced lets both projections run as one batched GEMM."""
        from .. import hipnp as hp
        ws = [self.gate.weight, self.up.weight]
        st = hp.stacked_view([w.data for w in ws])
        if st is not None and st._strides[0] == ws[0].data.size:      # already adjacent, gate first
            return
        buf = hp.empty((2,) + tuple(ws[0].shape), ws[0].dtype)
        for i, w in enumerate(ws):
            buf[i] = w.data
            w.data = buf[i]

    def forward(self, x, residual=None):
        if fused.ffn_swiglu.applicable(x, self.gate.weight, self.up.weight, self.down.weight):
            # the whole block as one node: SwiGLU forward / backward ride in the projections' epilogues
            return fused.ffn_swiglu(x, self.gate.weight, self.up.weight, self.down.weight, residual)
        if fused.gate_up_swiglu.applicable(x, self.gate.weight, self.up.weight):
            h = fused.gate_up_swiglu(x, self.gate.weight, self.up.weight)
        else:
            h = fused.swiglu(self.gate(x), self.up(x))
        if residual is None:
            return self.down(h)
        return fused.linear(h, self.down.weight, None, residual)      # residual add in the GEMM epilogue


class Attention(nn.Module):
    def __init__(self, dim, n_heads, max_seq_len, max_batch_size=None, dtype=None):
        super().__init__()
        assert dim % n_heads == 0
        self.dim, self.n_heads, self.head_dim = dim, n_heads, dim // n_heads
        self.Q = nn.Linear(dim, dim, bias=False, dtype=dtype)
        self.K = nn.Linear(dim, dim, bias=False, dtype=dtype)
        self.V = nn.Linear(dim, dim, bias=False, dtype=dtype)
        self.O = nn.Linear(dim, dim, bias=False, dtype=dtype)
        self.max_seq_len = max_seq_len
        self.max_batch_size = max_batch_size if max_batch_size is not None else 1
        shape = (self.max_batch_size, max_seq_len, n_heads, self.head_dim)
        self.cache_k = nn.Parameter(zeros(shape, dtype=dtype), requires_grad=False)
        self.cache_v = nn.Parameter(zeros(shape, dtype=dtype), requires_grad=False)

    def move(self, device):
        super().move(device)
        if device.is_hip:
            self._pack_qkv()
        return self

    def _pack_qkv(self):
        """Re-home the Q/K/V weights in one (3, dim, dim) buffer: each stays a contiguous Parameter,
        and being equally spaced lets the three projections run as one batched GEMM."""
        from .. import hipnp as hp
        ws = [self.Q.weight, self.K.weight, self.V.weight]
        st = hp.stacked_view([w.data for w in ws])
        if st is not None and st._strides[0] == ws[0].data.size:      # already adjacent, in order
            return
        buf = hp.empty((3,) + tuple(ws[0].shape), ws[0].dtype)
        for i, w in enumerate(ws):
            buf[i] = w.data
            w.data = buf[i]

    def __call__(self, x, start_pos, mask, freqs_cos, freqs_sin, residual=None):
        B, L, _ = x.shape
        H, hd = self.n_heads, self.head_dim
        if (self._train and start_pos == 0 and mask is not None and is_grad_enable()
                and fused.qkv_attention.applicable(x, L, hd)):
            out = fused.qkv_attention(x, self.Q.weight, self.K.weight, self.V.weight, freqs_cos, freqs_sin, H)
            out = out.reshape(B, L, -1)
            if residual is None:
                return self.O(out)
            return fused.linear(out, self.O.weight, None, residual)
        xq = self.Q(x).reshape(B, L, H, hd)
        xk = self.K(x).reshape(B, L, H, hd)
        xv = self.V(x).reshape(B, L, H, hd)
        xq, xk = apply_rotary_emb(xq, xk, freqs_cos, freqs_sin)
        if not self._train:                       # KV cache: inference only (model.py:105-110)
            self.cache_k[:B, start_pos:start_pos + L] = xk
            self.cache_v[:B, start_pos:start_pos + L] = xv
            xk = self.cache_k[:B, :start_pos + L]
            xv = self.cache_v[:B, :start_pos + L]
        out = fused.attention(xq, xk, xv, causal=mask is not None, start_pos=start_pos)
        out = out.reshape(B, L, -1)
        if residual is None:
            return self.O(out)
        return fused.linear(out, self.O.weight, None, residual)


    def step_rows(self, x, pos, freqs_cos, freqs_sin, residual=None):
        """One new token per row, row b at its own position pos[b] (Llama.generate_ragged; pos[b] < 0: a stopped row,
        computed at position 0 and its cache left alone).  Built from the operators above: RoPE with the cos / sin row of
        each row's position, the cache written at (b, pos[b]), attention over the cache with -inf for keys j > pos[b]."""
        B = x.shape[0]
        H, hd = self.n_heads, self.head_dim
        p = np.maximum(pos, 0)
        xq = self.Q(x).reshape(B, 1, H, hd)
        xk = self.K(x).reshape(B, 1, H, hd)
        xv = self.V(x).reshape(B, 1, H, hd)
        # the B rows as one sequence of B positions: RoPE takes one (cos, sin) row per position
        cos, sin = freqs_cos[p], freqs_sin[p]
        xq = fused.rope(xq.reshape(1, B, H, hd), cos, sin).reshape(B, 1, H, hd)
        xk = fused.rope(xk.reshape(1, B, H, hd), cos, sin).reshape(B, 1, H, hd)
        for b in np.flatnonzero(pos >= 0):
            self.cache_k[int(b), int(p[b])] = xk[int(b), 0]
            self.cache_v[int(b), int(p[b])] = xv[int(b), 0]
        T = int(p.max()) + 1
        mask = np.where(np.arange(T)[None, :] > p[:, None], -np.inf, 0.0).astype(xq.dtype).reshape(B, 1, 1, T)
        out = fused.attention(xq, self.cache_k[:B, :T], self.cache_v[:B, :T], causal=False, mask=mask)
        out = out.reshape(B, 1, -1)
        if residual is None:
            return self.O(out)
        return fused.linear(out, self.O.weight, None, residual)


class TransformerBlock(nn.Module):
    def __init__(self, dim, n_heads, ffn_dim, max_seq_len, max_batch_size=None, dtype=None):
        super().__init__()
        self.attention = Attention(dim, n_heads, max_seq_len, max_batch_size, dtype)
        self.ffn = FeedForward(dim, ffn_dim, dtype)
        self.input_norm = nn.RMSNorm(dim, dtype=dtype)
        self.post_attn_norm = nn.RMSNorm(dim, dtype=dtype)

    def forward(self, x, start_pos, mask, freqs_cos, freqs_sin):
        # z = x + attn(norm(x)); out = z + ffn(norm(z)) -- both adds ride in the GEMM epilogues
        z = self.attention(self.input_norm(x), start_pos, mask, freqs_cos, freqs_sin, residual=x)
        return self.ffn(self.post_attn_norm(z), residual=z)

    def step_rows(self, x, pos, freqs_cos, freqs_sin):
        z = self.attention.step_rows(self.input_norm(x), pos, freqs_cos, freqs_sin, residual=x)
        return self.ffn(self.post_attn_norm(z), residual=z)


class Llama(nn.Module):
    def __init__(self, vocab_size, embed_dim, n_heads, ffn_dim, max_seq_len, max_batch_size=None,
                 n_layers=6, dtype=None):
        super().__init__()
        self.vocab_size, self.embed_dim, self.n_heads, self.ffn_dim = vocab_size, embed_dim, n_heads, ffn_dim
        self.max_seq_len, self.max_batch_size, self.n_layers = max_seq_len, max_batch_size, n_layers
        self.tok_embedding = nn.Embedding(vocab_size, embed_dim, dtype=dtype)
        cos, sin = compute_cos_sin_cache(embed_dim // n_heads, max_seq_len, dtype=dtype)
        self.freqs_cos = nn.Parameter(cos, False)
        self.freqs_sin = nn.Parameter(sin, False)
        self.layers = nn.ModuleList([
            TransformerBlock(embed_dim, n_heads, ffn_dim, max_seq_len, max_batch_size, dtype)
            for _ in range(n_layers)])
        self.norm = nn.RMSNorm(embed_dim, dtype=dtype)
        self.lm_head = nn.Linear(embed_dim, vocab_size, dtype=dtype)      # bias=True, as the reference

    def _forward_hidden(self, input_ids, start_pos: int):
        L = input_ids.shape[-1]
        h = self.tok_embedding(input_ids)
        cos = self.freqs_cos[start_pos:start_pos + L]
        sin = self.freqs_sin[start_pos:start_pos + L]
        # the reference rebuilds an additive -inf mask on the host every call (model.py:199-203);
        # here causality is a flag of the fused attention node and nothing is uploaded.
        mask = True if L > 1 else None
        for layer in self.layers:
            h = layer(h, start_pos, mask, cos, sin)
        return self.norm(h)

    def forward_logits(self, input_ids, start_pos: int = 0):
        return self.lm_head(self._forward_hidden(input_ids, start_pos))

    def set_trainable_parameters(self, trainable_prefixes=("lm_head",)):
        trainable = frozen = 0
        for name, p in self._parameters.items():
            p.requires_grad = any(name.startswith(pre) for pre in trainable_prefixes)
            trainable, frozen = trainable + p.requires_grad, frozen + (not p.requires_grad)
        return trainable, frozen

    def loss(self, input_ids, target_ids, criterion=None, start_pos: int = 0):
        h = self._forward_hidden(input_ids, start_pos)
        if isinstance(target_ids, Tensor):
            targets = target_ids.reshape(-1)
        else:
            targets = Tensor(np.asarray(target_ids).reshape(-1), dtype=np.int64, device=h.device)
        head = self.lm_head
        bias = getattr(head, "bias", None)
        reduction = getattr(criterion, "reduction", "mean") if criterion is not None else "mean"
        if ((criterion is None or type(criterion) is nn.CrossEntropyLoss) and type(head) is nn.Linear
                and fused.linear_cross_entropy.applicable(h, head.weight, bias, targets, reduction)):
            # lm_head + cross entropy as one node: the (tokens, vocab) gradient of the logits is never written
            return fused.linear_cross_entropy(h, head.weight, bias, targets, reduction)
        logits = head(h)
        B, L, V = logits.shape
        return (criterion or nn.CrossEntropyLoss())(logits.reshape(B * L, V), targets)

    def finetune_step(self, input_ids, target_ids, optimizer, criterion=None, start_pos: int = 0):
        """zero_grad -> forward -> cross entropy -> backward -> optimizer step; returns the loss."""
        self.train(True)
        optimizer.zero_grad()
        loss = self.loss(input_ids, target_ids, criterion, start_pos)
        loss.backward()
        optimizer.step()
        return loss.item()

    def forward(self, input_ids, start_pos: int):
        return self.lm_head(self._forward_hidden(input_ids, start_pos)[:, [-1], :])

    fast_decode = True      # class switch: False keeps every decode step on the generic tape-node path

    def generate(self, input_ids, max_new_tokens: int, temperature=0.0, top_k=0, top_p=1.0, seed=0,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logprobs=None):
        """Yield the next ids, (B, 1) int64, for positions L .. max_new_tokens - 1.  temperature 0 (the default): the
        greedy pick of the reference (model.py:258-269); temperature > 0: drawn with top-k / top-p and the seeded
        counter-based generator of llm/sampling.py (token at position t of row b: Philox counter (t, b)).
        `repetition_penalty` / `presence_penalty` / `frequency_penalty` (defaults: off): the penalties of llm/penalties.py
        on each row's logits -- its prompt's tokens and the tokens it generated -- before the pick or the draw.
        `logprobs` = n (an int in [0, 20]; None: off): every step yields (ids, lp) instead, lp an llm/logprobs.Logprobs
        of the row the pick or the draw read -- token (B, 1), top_ids (B, n), top_logprobs (B, n).  The arguments are
        checked here, before anything runs."""
        temperature, top_k, top_p, seed = check_sampling_args(temperature, top_k, top_p, seed)
        penalty = pen_np.check_args(repetition_penalty, presence_penalty, frequency_penalty)
        n_lp = lp_np.check_n(logprobs)
        return self._generate(input_ids, max_new_tokens, (temperature, top_k, top_p, seed) if temperature > 0 else None,
                              penalty, n_lp)

    def _generate(self, input_ids, max_new_tokens, sampling, penalty=None, n_lp=None):
        B, L = input_ids.shape
        next_id = None
        pen = None
        if penalty is not None:                                   # (the rows' prompts and counts: llm/penalties.py)
            ids = np.asarray(input_ids.numpy() if isinstance(input_ids, Tensor) else input_ids).reshape(B, L)
            pen = pen_np.Rows(B, self.vocab_size, penalty, list(ids))
        for i, pos in enumerate(range(L, max_new_tokens)):
            if i == 0:
                logits = self(input_ids, 0)[:, -1, :]             # prompt pass: fills the KV caches
                if pen is not None:
                    logits = self._penalize_prompt(logits, pen.prompts, penalty)
                next_id = logits.argmax(-1, True) if sampling is None else sample_next(logits, pos, *sampling)
                lp = None if n_lp is None else self._logprobs_rows(logits, next_id.numpy(), n_lp)
            elif (Llama.fast_decode and next_id.device.is_hip and not self._train
                  and self.lm_head.weight.dtype == np.float32 and (self.embed_dim // self.n_heads) % 4 == 0):
                # (`more`: another token will be asked for -- the step after this one may be queued ahead)
                out = self._decode_step_hip(next_id.data, pos, more=pos + 1 < max_new_tokens, sampling=sampling,
                                            pen=pen, n_lp=n_lp)
                out, lp = out if n_lp is not None else (out, None)
                next_id = Tensor(out, dtype=np.int64, device=next_id.device, copy=False)
            else:
                logits = self(next_id, pos)[:, -1, :]
                if pen is not None:
                    logits = self._penalize_step(logits, pen, next_id.numpy(), np.full(B, pos))
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

    def score(self, input_ids, logprobs=0):
        """log p(x_t | x_<t) of given sequences: input_ids (B, L) int, L >= 2.  Returns llm/logprobs.Logprobs for
        positions 1 .. L-1: token (B, L-1), top_ids / top_logprobs (B, L-1, n) for `logprobs` = n in [0, 20].  One forward
        pass (`forward_logits`) in training mode under no_grad -- training mode writes no KV cache, so neither the cache
        nor max_batch_size bounds it -- then the module's mode is restored.  Arguments are checked before anything runs.
        Against the values generation reports: the first generated token (the prompt's causal pass) agrees; later ones
        need not, since a decode step of `generate` at position p feeds the token of position p - 1 (as the reference
        does) and attends to a never-written cache slot, so it is not a causal pass over prompt + generated tokens."""
        from ..autograd import no_grad
        n = lp_np.check_n(logprobs, allow_none=False)
        ids = np.asarray(input_ids.numpy() if isinstance(input_ids, Tensor) else input_ids)
        if ids.ndim != 2 or ids.shape[1] < 2:
            raise ValueError(f"score takes (B, L) token ids with L >= 2, got shape {ids.shape}")
        if ids.size and (ids.dtype.kind not in "iu" or ids.min() < 0 or ids.max() >= self.vocab_size):
            raise ValueError(f"token ids must be integers in [0, {self.vocab_size})")
        B, L = ids.shape
        if L - 1 > self.freqs_cos.shape[0]:
            raise ValueError(f"score: {L - 1} positions exceed the RoPE table's {self.freqs_cos.shape[0]} rows")
        ids = ids.astype(np.int64)
        mode = self._train
        dev = self.tok_embedding.weight.device
        try:
            self.train(True)
            with no_grad():
                logits = self.forward_logits(Tensor(ids[:, :-1], dtype=np.int64, device=dev), 0)
                lp = self._logprobs_rows(logits.reshape(B * (L - 1), self.vocab_size), ids[:, 1:].reshape(-1), n)
        finally:
            self.train(mode)
        return lp_np.Logprobs(lp.token.reshape(B, L - 1), lp.top_ids.reshape(B, L - 1, n),
                              lp.top_logprobs.reshape(B, L - 1, n))

    def generate_ragged(self, prompts, max_new_tokens: int, temperature=0.0, top_k=0, top_p=1.0, seed=0, stop_ids=(),
                        speculate=0, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                        logprobs=None):
        """Generation for B prompts of different lengths, every row at its own position.  Yields a (B, 1) int64 Tensor
        per step: step i holds, for row b, the token at position len_b + i.  `max_new_tokens` is the number of NEW tokens
        per row -- `generate`'s second argument is an end position instead: for equal lengths L,
        `generate_ragged(rows, n)` yields what `generate(ids, L + n)` yields.  Sampling follows llm/sampling.py with
        the row's own position as the counter: row b's token at position t is drawn with counter (t, b).
        `stop_ids`: once row b yields one of them it yields -1 at every later step and its position stops advancing
        (its KV cache is no longer written); the iterator ends after the step at which every row has stopped, or after
        `max_new_tokens` steps.  `speculate` = k > 0: prompt-lookup speculative decoding (llm/speculative.py) -- up to k
        draft tokens per row per target pass, each checked against the token the model picks at its position.  On `cpu`
        (and every path that verifies through the one-token rows step) the steps yielded are those of `speculate=0`; the
        graph-replayed HIP pass computes the logits with other kernels than the plain step (the wide product, the extend
        attention), so there they agree up to fp32 near-ties, as the plain step and the wide step do.  The counts of the
        run are in `last_speculation` (None after a call with speculate=0, which runs the plain decode).
        `repetition_penalty` / `presence_penalty` / `frequency_penalty`: as in `generate` (llm/penalties.py), row b's
        prompt and generated tokens; not with speculate > 0.
        `logprobs` = n: as in `generate`, every step yields (ids, lp); a row that yields -1 has nan / -1 / nan.  Not with
        speculate > 0.
        Every argument is checked here (ValueError), before anything runs."""
        temperature, top_k, top_p, seed = check_sampling_args(temperature, top_k, top_p, seed)
        V = self.vocab_size
        if int(max_new_tokens) != max_new_tokens or max_new_tokens < 0:
            raise ValueError(f"max_new_tokens must be a non-negative integer, got {max_new_tokens}")
        max_new_tokens = int(max_new_tokens)
        rows = [np.asarray(p.numpy() if isinstance(p, Tensor) else p).reshape(-1) for p in prompts]
        cache = self.layers[0].attention.cache_k
        if not rows:
            raise ValueError("generate_ragged needs at least one prompt")
        k = spec_np.check_speculate(speculate, len(rows))
        penalty = pen_np.check_args(repetition_penalty, presence_penalty, frequency_penalty, k)
        n_lp = lp_np.check_n(logprobs)
        if n_lp is not None and k:
            raise ValueError("logprobs are not available with speculate > 0")
        if len(rows) > cache.shape[0]:
            raise ValueError(f"batch {len(rows)} exceeds the KV cache's max_batch_size {cache.shape[0]}")
        limit = min(cache.shape[1], self.freqs_cos.shape[0])     # positions the cache / RoPE table hold
        for b, r in enumerate(rows):
            if r.size == 0:
                raise ValueError(f"prompt {b} is empty")
            if r.dtype.kind not in "iu" or r.min() < 0 or r.max() >= V:
                raise ValueError(f"prompt {b}: token ids must be integers in [0, {V})")
            last = r.size + max_new_tokens - 1                   # (the position of the row's last decode step)
            if r.size > cache.shape[1] or (max_new_tokens > 1 and last >= limit):
                raise ValueError(f"prompt {b}: its last position {last} is outside the KV cache / RoPE table "
                                 f"(max_seq_len {cache.shape[1]}, {self.freqs_cos.shape[0]} RoPE rows)")
        stops = np.asarray(sorted({int(t) for t in stop_ids}), np.int64)
        if stops.size and (stops.min() < 0 or stops.max() >= V):
            raise ValueError(f"stop ids must lie in [0, {V}), got {stops.tolist()}")
        sampling = (temperature, top_k, top_p, seed) if temperature > 0 else None
        self.last_speculation = None if k == 0 else spec_np.counts()
        if k:
            return self._speculate([r.astype(np.int64) for r in rows], max_new_tokens, k, sampling, stops)
        return self._generate_ragged([r.astype(np.int64) for r in rows], max_new_tokens, sampling, stops, penalty,
                                     n_lp)

    def _generate_ragged(self, rows, n, sampling, stops, penalty=None, n_lp=None):
        B = len(rows)
        lens = np.array([r.size for r in rows], np.int64)
        if n == 0:
            return
        pen = None if penalty is None else pen_np.Rows(B, self.vocab_size, penalty, rows)
        nxt = self._prompt_rows(rows, lens, sampling, penalty, n_lp)
        if n_lp is not None:
            nxt, lp = nxt
        live = np.ones(B, bool)
        if stops.size:
            live = ~np.isin(nxt.numpy().reshape(-1), stops)
        yield nxt if n_lp is None else (nxt, lp_np.as_step(lp))
        fast = (Llama.fast_decode and nxt.device.is_hip and not self._train
                and self.lm_head.weight.dtype == np.float32 and (self.embed_dim // self.n_heads) % 4 == 0)
        if fast:
            from .. import hipnp as hp
            mask = np.zeros(-(-self.vocab_size // 32), np.uint32)
            np.bitwise_or.at(mask, stops >> 5, np.uint32(1) << (stops & 31).astype(np.uint32))
            # tokens by STEP: slot i holds step i of every row (-1 for a stopped row), so "not written yet" is its own
            # value; two slots beyond the last step for the runs of a graph capture
            run = {"lens": lens, "live": live, "sampling": sampling, "stop_mask": mask.view(np.int32), "pen": pen,
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
                nxt = self._step_module_rows(nxt, np.where(live, lens + i, -1), sampling, pen=pen, n_lp=n_lp)
                nxt, lp = nxt if n_lp is not None else (nxt, None)
            if stops.size:
                yield nxt if n_lp is None else (nxt, lp_np.as_step(lp))
                tok = nxt.numpy().reshape(-1)                    # (fast path: a poll of the mapped history slot)
                live = live & (tok >= 0) & ~np.isin(tok, stops)
                continue
            yield nxt if n_lp is None else (nxt, lp_np.as_step(lp))

    def _prompt_rows(self, rows, lens, sampling, penalty=None, n_lp=None):
        """The prompt pass of a ragged generation: the prompts right-padded to the longest and run as one batched
        causal pass from position 0 (no real token attends to a pad after it); each row's logits at its last real token,
        gathered before lm_head.  The cache slots the pads wrote, [len_b, L_max) of row b, are put back as they were: a
        row's cache is written at its own positions only.  `penalty`: the logits penalised for each row's prompt first.
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
        nxt = logits.argmax(-1, True) if sampling is None else sample_next_rows(logits, lens, *sampling)
        if n_lp is None:
            return nxt
        return nxt, self._logprobs_rows(logits, nxt.numpy(), n_lp)

    def _step_module_rows(self, ids, pos, sampling, req=None, pen=None, n_lp=None):
        """One ragged decode step on the tape-node operators (the `cpu` device, fast_decode = False, training mode,
        other dtypes): row b's token at position pos[b] (-1: a stopped row, which yields -1).  The NumPy statement of what
        the per-row kernels compute.  `req`: the counter id of each row (Llama.serve; default: the row).  `pen`
        (llm/penalties.Rows): the fed tokens counted and the logits penalised before the pick.  `n_lp`: returns (ids,
        Logprobs of the rows, none for rows at -1)."""
        p = np.maximum(pos, 0)
        logits = self._step_logits_rows(ids, pos)
        if pen is not None:
            logits = self._penalize_step(logits, pen, ids.numpy(), pos)
        nxt = logits.argmax(-1, True) if sampling is None else sample_next_rows(logits, p, *sampling, rows=req)
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

    # -- decode fast path -----------------------------------------------------------
    graph_decode = True     # class switch: False issues the step's launches one by one instead of replaying a hipGraph
    decode_ahead = True     # class switch: False never queues the next step before the caller asked for it
    last_speculation = None  # the counts of the last generate_ragged(speculate=k > 0) run (llm/speculative.py)
    fused_decode = 2        # class switch: launches per layer = 2 (q|k|v inside the attention kernel), 1 -> 3, 0 / False -> 5
    wide_decode = True      # class switch: 9 .. 256 rows on the wide step (csrc/decode_wide.hip); False -> the generic step

    def _decode_plan(self, B, sampling=False, ragged=False, serve=False, beam=0, n_stops=0, penalty=False, n_lp=None):
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
        slots of mapped host memory (`lp_box`, reached through the device pointer `lp_ptr`)."""
        from .. import hipnp as hp, _lib
        D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        st = getattr(self, "_decode_st", None)
        # a captured step (and the stacked weight views) hold the address of EVERY array the launches read: the key
        # covers them all -- rebinding `.data` of any parameter / cache re-plans -- and the switches that shape the plan
        ptrs = self._weight_ptrs()
        cache_len = self.layers[0].attention.cache_k.shape[1]
        wide = B > 8 and Llama.wide_decode and self._decode_wide_ok(B, cache_len)
        key = (B, hp._state["device"], int(Llama.fused_decode or 0), os.environ.get("PDN_DECODE_SPLITS", ""),
               cache_len, tuple(ptrs), bool(sampling), wide,   # (the addresses: no hash to collide)
               (int(beam), int(n_stops), bool(penalty)), bool(ragged), bool(serve)) + (() if n_lp is None else (int(n_lp),))
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
              "wide": wide, "rows": bool(ragged or wide), "beam": int(beam), "full": bool(sampling or beam or penalty),
              "pen": bool(penalty), "lp_n": n_lp}
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
                      params=hp.zeros((3,), np.int64) if sampling else None, params_val=None,
                      **{n: hp.empty((B, w), np.float32) for n, w in
                         (("x", D), ("qkv", 3 * D), ("att", ns * H * (4 + D // H)), ("gu", 2 * F), ("logits", V))})
            # three launches per layer (csrc/decode_layer.hip): the output / down projections leave per-head /
            # per-32-hidden-unit records that the next kernel's staging adds to the residual row
            J = _lib.lib().query("pdn_decode_mlp_slices", F)
            st["fused"] = bool(not wide and Llama.fused_decode and J and D <= 1024 and ns * H <= 256 and len(self.layers) > 0 and all(
                l.ffn.gate.weight.data.is_contiguous() and l.ffn.up.weight.data.is_contiguous() for l in self.layers))
            # two launches per layer (csrc/decode_block.hip): the q | k | v projection inside the attention kernel, one
            # more record per head for the new key
            st["block"] = bool(st["fused"] and int(Llama.fused_decode) >= 2 and
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
        head = self.lm_head
        bias = head.bias.data._ptr if getattr(head, "bias", None) is not None else None
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
            self._decode_tick(st, s)
            self._lp_tick(st, s)
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
        self._decode_tick(st, s)
        self._lp_tick(st, s)

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
        head = self.lm_head
        bias = head.bias.data._ptr if getattr(head, "bias", None) is not None else None
        cv, ci = (None, None) if st["full"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        L.call("pdn_decode_wide_gemm_f32", x, D, 1, self.norm.weight.data._ptr, self.norm.eps, 0, 0, head.weight.data._ptr,
               V, V, 0, bias, logits, V, 0 if st["full"] else 2, cv, ci, pos, B, D, V, work, s)
        self._pen_step(st, s)
        self._decode_tick(st, s)
        self._lp_tick(st, s)

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

    def _lp_begin(self, st):
        """A fresh record ring for a new generation (stream ordered, as the history pointer)."""
        from .. import hipnp as hp
        if st.get("lp_n") is None:
            return
        st["lp_box"] = hp.Mailbox(_LP_RING, (st["B"], lp_np.record_words(st["lp_n"])), unset=lp_np.UNSET)
        st["lp_ptr"][...] = np.int64(st["lp_box"]._ptr)

    def _lp_scratch(self, st):
        """During a graph capture the record pointer goes to a scratch ring (as the history's); returns the restore."""
        from .. import hipnp as hp
        if st.get("lp_n") is None:
            return lambda: None
        scratch = hp.Mailbox(_LP_RING, (st["B"], lp_np.record_words(st["lp_n"])), unset=lp_np.UNSET)
        st["lp_ptr"][...] = np.int64(scratch._ptr)

        def restore(keep=scratch):                         # (the scratch lives until the capture's runs are done)
            st["lp_ptr"][...] = np.int64(st["lp_box"]._ptr)
        return restore

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
        cv, ci = (None, None) if st["sampling"] else (st["cand_v"]._ptr, st["cand_i"]._ptr)
        _lib.lib().call("pdn_penalty_step_f32", st["logits"]._ptr, V, B, V, st["pen_params"]._ptr, st["counts"]._ptr,
                        st["seen"]._ptr, st["start"]._ptr, st["ids"]._ptr, st["pos"]._ptr, int(st["rows"]), cv, ci, s)

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

    def _decode_tick(self, st, s):
        """The last launch of a step: the greedy pick over the projection's candidates, or (sampling plans) the sample
        tick over the full logit rows with counter (*pos, b); either stores the token and its embedding row, *pos += 1."""
        from .. import _lib
        L, emb, D, B = _lib.lib(), self.tok_embedding.weight.data, self.embed_dim, st["B"]
        if st["beam"]:
            self._beam_launches(st["bm"], st["logits"]._ptr, self.vocab_size, st["pos"]._ptr, st["step"]._ptr,
                                st["ids"]._ptr, st["x"]._ptr, first=False)
            return
        if st["wide"]:
            # (one workgroup per row: the last row to finish advances the step counter, csrc/decode_wide.hip)
            cnt = (st["pos"]._ptr, st["step"]._ptr, st["arrive"]._ptr)
            out = (st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D, st["x"]._ptr, s)
            src = ((st["logits"]._ptr, self.vocab_size, B, self.vocab_size, st["params"]._ptr) if st["sampling"] else
                   (st["cand_v"]._ptr, st["cand_i"]._ptr, B, st["cand_v"].shape[1]))
            kind = "sample" if st["sampling"] else "pick"
            if st["serve"]:
                L.call(f"pdn_decode_wide_{kind}_tick_slots_f32", *src, st["ids"]._ptr, *cnt, st["req"]._ptr,
                       st["left"]._ptr, st["ring"], st["stop"]._ptr, *out)
            else:
                L.call(f"pdn_decode_wide_{kind}_tick_rows_f32", *src, st["ids"]._ptr, *cnt, st["stop"]._ptr, *out)
            return
        if st["serve"]:
            # (the slot ticks: counter (pos[b], req[b]), a token budget per row, a history ring)
            srv = (st["pos"]._ptr, st["step"]._ptr, st["req"]._ptr, st["left"]._ptr, st["ring"], st["stop"]._ptr,
                   st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D, st["x"]._ptr, s)
            if st["sampling"]:
                L.call("pdn_decode_sample_tick_slots_f32", st["logits"]._ptr, self.vocab_size, B, self.vocab_size,
                       st["params"]._ptr, st["ids"]._ptr, *srv)
            else:
                L.call("pdn_decode_pick_tick_slots_f32", st["cand_v"]._ptr, st["cand_i"]._ptr, B, st["cand_v"].shape[1],
                       st["ids"]._ptr, *srv)
            return
        if st["ragged"]:
            pos, step, stop = st["pos"]._ptr, st["step"]._ptr, st["stop"]._ptr
            if st["sampling"]:
                L.call("pdn_decode_sample_tick_rows_f32", st["logits"]._ptr, self.vocab_size, B, self.vocab_size,
                       st["params"]._ptr, st["ids"]._ptr, pos, step, stop, st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D,
                       st["x"]._ptr, s)
            else:
                L.call("pdn_decode_pick_tick_rows_f32", st["cand_v"]._ptr, st["cand_i"]._ptr, B, st["cand_v"].shape[1],
                       st["ids"]._ptr, pos, step, stop, st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D, st["x"]._ptr, s)
            return
        if st["sampling"]:
            L.call("pdn_decode_sample_tick_f32", st["logits"]._ptr, self.vocab_size, B, self.vocab_size, st["params"]._ptr,
                   st["ids"]._ptr, st["pos"]._ptr, st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D, st["x"]._ptr, s)
            return
        L.call("pdn_decode_pick_tick_f32", st["cand_v"]._ptr, st["cand_i"]._ptr, B, st["cand_v"].shape[1],
               st["ids"]._ptr, st["pos"]._ptr, st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D, st["x"]._ptr, s)

    def _decode_gather(self, st):
        """x = tok_embedding[ids] for ids that did not come out of the previous step's pick kernel."""
        from .. import hipnp as hp, _lib
        emb = self.tok_embedding.weight.data
        _lib.lib().call("pdn_embedding_gather_f32", emb._ptr, self.vocab_size, self.embed_dim, emb._strides[0],
                        st["ids"]._ptr, st["B"], st["x"]._ptr, hp.err_flag_ptr(), hp.stream())

    def _decode_step_hip(self, ids, pos: int, more: bool = False, sampling=None, pen=None, n_lp=None):
        """One decode step (one new token per sequence) without building tape nodes.  ids: (B, 1) int64
        device array; returns the next ids, (B, 1) int64.  The step is ONE hipGraph replay: norm + projection,
        RoPE + cache append, decode attention, SwiGLU + down projection and the greedy pick all read the position
        from device memory (csrc/decode.hip), so nothing changes between replays but the data.  `sampling`: None =
        greedy, else (temperature, top_k, top_p, seed) and the step ends in the sample tick (csrc/sample.hip).  `pen`
        (llm/penalties.Rows of this generation, or None): a penalty plan; its rows are reset from the prompts when a new
        generation begins.  `n_lp`: returns (ids, Logprobs of the step)."""
        from .. import hipnp as hp, _lib
        B = ids.shape[0]
        cache = self.layers[0].attention.cache_k
        # raw pointers / device-side offsets are formed from `pos`: refuse what the module path would also refuse
        # (the reference fails with a NumPy broadcast error, model.py:105-110)
        if pos < 0 or pos >= cache.shape[1] or pos >= self.freqs_cos.shape[0]:
            raise ValueError(f"decode position {pos} is outside the KV cache / RoPE table "
                             f"(max_seq_len {cache.shape[1]}, {self.freqs_cos.shape[0]} RoPE rows)")
        if B > cache.shape[0]:
            raise ValueError(f"batch {B} exceeds the KV cache's max_batch_size {cache.shape[0]}")
        st = self._decode_plan(B, sampling is not None, penalty=pen is not None, n_lp=n_lp)
        if st is None:
            return self._decode_step_generic(ids, pos, sampling, pen, n_lp)
        ahead, st["ahead"] = st.get("ahead"), None
        if ahead is not None:
            if (ahead[0] == pos and ahead[1] is ids and st["params_val"] == sampling     # exactly this step, queued ahead
                    and st.get("pen_run") is pen):
                out = st["last_out"] = ahead[2]
                if more and Llama.decode_ahead and pos + 1 < min(cache.shape[1], self.freqs_cos.shape[0]):
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
            st["hist_ptr"][...] = np.int64(st["hist"]._ptr)
            self._lp_begin(st)
        if st["params_val"] != sampling:
            if sampling is not None:
                st["params"][...] = params_bytes(*sampling)      # (stream-ordered: earlier steps read the old values)
            st["params_val"] = sampling
        if pen is not None and st["pen_run"] is not pen:         # a new generation: its rows' prompts, zero counts
            self._pen_reset(st, np.arange(B), pen.prompts, pen.values)
            st["pen_run"] = pen
        fresh = ids is not st["ids"] and ids is not st.get("last_out")
        if fresh:
            st["ids"][...] = ids                                 # (not the array the previous step returned: that
            self._decode_gather(st)                              # one's embedding row is already in x)
        ns = self._decode_ns(st, pos)
        g = False if st["nograph"] else st["graphs"].get((ns, st["sampling"]))
        if g is None and Llama.graph_decode and pos + 2 < min(cache.shape[1], self.freqs_cos.shape[0]):
            # capture once: hipnp.Graph runs the step twice for real (pool warm-up + first replay), which writes the
            # cache rows of positions pos and pos + 1 with exactly what the real steps will write there; the
            # position and the ids are then put back and the real step replayed
            # The pick kernel of those two runs stores its tokens into the history: it is pointed at a SCRATCH
            # history meanwhile, so that slots pos / pos + 1 of the real one stay "not written" (-1) until the real
            # steps store there (a later step with other ids would otherwise read the capture's token as its own).
            keep = st["ids"].copy()
            counts = st["counts"].copy() if st["pen"] else None  # (the capture's runs count their fed tokens too)
            scratch = hp.Mailbox(cache.shape[1], (B, 1))
            st["hist_ptr"][...] = np.int64(scratch._ptr)
            lp_restore = self._lp_scratch(st)
            try:
                g = hp.Graph()
                g.capture(lambda: self._decode_launches(st, ns))
                st["graphs"][(ns, st["sampling"])] = g
            except _lib.HipLibraryError as e:
                if e.code != -2:                                 # PDN_EUNSUPPORTED: no graph support (the emulated
                    raise                                        # ABI) -> plain launches; anything else is a bug
                st["nograph"], g = True, False
            hp.synchronize()                                     # the capture's runs are done with the scratch history
            st["hist_ptr"][...] = np.int64(st["hist"]._ptr)
            lp_restore()
            st["pos"][...] = np.int32(pos)
            if st["rows"]:
                st["step"][...] = np.int32(pos)
            st["ids"][...] = keep
            if counts is not None:
                st["counts"][...] = counts
            self._decode_gather(st)
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
        st["host_pos"] = pos + 1
        # the caller's own array = this position's slot of the history (host memory the GPU writes): reading the token
        # polls THAT slot only -- no copy command, no event -- while the compute stream may already run the next step
        out = st["last_out"] = st["hist"].slot(pos)
        if (more and Llama.decode_ahead and (st["graphs"] or st["nograph"])
                and pos + 1 < min(cache.shape[1], self.freqs_cos.shape[0])):
            self._decode_ahead(st, pos + 1)
        return out if n_lp is None else (out, self._lp_read(st, pos))

    def _decode_ahead(self, st, pos):
        """Queue the step of position `pos` right behind the one just issued -- its input ids are already where the
        gather reads them -- so the GPU does not idle while the host hands the previous token to the caller.  The
        result is kept for the next `_decode_step_hip(last_out, pos)` call; any other call discards it."""
        ns = self._decode_ns(st, pos)
        g = False if st["nograph"] else st["graphs"].get((ns, st["sampling"]))
        if g is None:
            return                                               # (a new range count: its step is captured by the next call)
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
        st["host_pos"] = pos + 1
        prev = st["last_out"]
        st["ahead"] = (pos, prev, st["hist"].slot(pos))

    def _decode_step_generic(self, ids, pos: int, sampling=None, pen=None, n_lp=None):
        """The same step from the library's generic entry points (skinny `pdn_gemm_f32`, RMSNorm, RoPE, decode
        attention, SwiGLU), ~77 launches from preallocated buffers: for shapes / layouts the graph path does not take."""
        from .. import hipnp as hp, _lib
        L, st = _lib.lib(), hp.stream()
        D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        hd, half = D // H, D // H // 2
        B = ids.shape[0]
        ws = getattr(self, "_decode_ws", None)
        if ws is None or ws["x"].device_index != hp._state["device"] or ws["x"].shape[0] != B:
            ws = {n: hp.empty((B, w), np.float32) for n, w in
                  (("x", D), ("h", D), ("q", D), ("att", D), ("g", F), ("u", F), ("sw", F), ("logits", V))}
            self._decode_ws = ws
        x, h, q, att, g, u, sw, logits = (ws[n]._ptr for n in ("x", "h", "q", "att", "g", "u", "sw", "logits"))

        def gemv(a_ptr, K, w, c_ptr, N, beta=0.0, bias=None, ldc=None):
            wd = w.data
            L.call("pdn_gemm_f32", B, N, K, 1.0, a_ptr, K, 1, wd._ptr, wd._strides[0], wd._strides[1], beta, c_ptr,
                   N if ldc is None else ldc, bias, 1, 1, 0, 0, 0, 0, 0, 0, None, None, 0, None, 0, st)

        emb = self.tok_embedding.weight.data
        idc = ids if ids.is_contiguous() else ids.copy()
        L.call("pdn_embedding_gather_f32", emb._ptr, V, D, emb._strides[0], idc._ptr, B, x, hp.err_flag_ptr(), st)
        cos = self.freqs_cos.data._ptr + pos * half * 4
        sin = self.freqs_sin.data._ptr + pos * half * 4
        for layer in self.layers:
            a, f = layer.attention, layer.ffn
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
            gemv(att, D, a.O.weight, x, D, beta=1.0)                      # x += att @ Wo
            L.call("pdn_rmsnorm_fwd_f32", x, layer.post_attn_norm.weight.data._ptr, h, None, B, D,
                   layer.post_attn_norm.eps, st)
            gemv(h, D, f.gate.weight, g, F)
            gemv(h, D, f.up.weight, u, F)
            L.call("pdn_swiglu_fwd_f32", g, u, sw, B * F, st)
            gemv(sw, F, f.down.weight, x, D, beta=1.0)                    # x += swiglu @ Wdown
        L.call("pdn_rmsnorm_fwd_f32", x, self.norm.weight.data._ptr, h, None, B, D, self.norm.eps, st)
        gemv(h, D, self.lm_head.weight, logits, V,
             bias=self.lm_head.bias.data._ptr if getattr(self.lm_head, "bias", None) is not None else None)
        if pen is not None:                           # (the statement of llm/penalties.py on the host counts)
            pen.feed(ids.get(), np.full(B, pos))
            ws["logits"][...] = pen.apply(ws["logits"].get())
        if sampling is None:
            out = ws["logits"].argmax(-1, keepdims=True)
        else:
            out = hp.empty((B, 1), np.int64)          # (the sampled form of the pick: counter (pos, b))
            L.call("pdn_sample_rows_f32", logits, V, B, V, params_buffer(*sampling)._ptr, pos, out._ptr, st)
        if n_lp is None:
            return out
        return out, self._logprobs_rows(ws["logits"], out.get(), n_lp)

    # -- ragged decode (generate_ragged): every row at its own position ------------------------------
    def _decode_step_rows(self, ids, run, i: int, more: bool = False):
        """Step i >= 1 of a ragged generation: row b's token at position lens[b] + i, rows the host knows to have stopped
        at -1.  ids: (B, 1) int64 device array (the previous step's tokens); returns this step's tokens, (B, 1) int64, -1
        for rows stopped before it.  The graph path of `_decode_step_hip` with the *_rows_f32 launches: the positions, the
        step counter and the stop bitmask live on the device, the history is indexed by the step (`run["hist"]`), and the
        range count follows the furthest row, max_b lens[b] + i, which the host knows without a device read."""
        from .. import hipnp as hp, _lib
        lens, live, sampling = run["lens"], run["live"], run["sampling"]
        B, top = len(lens), int(lens.max()) + i
        cache = self.layers[0].attention.cache_k
        limit = min(cache.shape[1], self.freqs_cos.shape[0])
        pos = np.where(live, lens + i, -1).astype(np.int32)
        n_lp = run.get("lp")
        st = self._decode_plan(B, sampling is not None, ragged=True, penalty=run.get("pen") is not None, n_lp=n_lp)
        if st is None:
            out = self._decode_step_generic_rows(ids, pos, sampling, pen=run.get("pen"), n_lp=n_lp)
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
                if more and Llama.decode_ahead and top + 1 < limit:
                    self._decode_ahead_rows(st, run, i + 1)
                return out if n_lp is None else (out, self._lp_read(st, i))
            hp.synchronize()                                     # a different request: the queued step is void
            st["host_step"] = st["last_out"] = None
        if st["run"] is not run or st["host_step"] != i:
            st["run"] = run                                      # (later steps: the device advances pos and step itself)
            st["pos"][...] = pos
            st["step"][...] = np.int32(i)
            st["stop"][...] = run["stop_mask"]
            st["hist_ptr"][...] = np.int64(run["hist"]._ptr)
            self._lp_begin(st)
        if st["params_val"] != sampling:
            if sampling is not None:
                st["params"][...] = params_bytes(*sampling)
            st["params_val"] = sampling
        pen = run.get("pen")
        if pen is not None and st["pen_run"] is not pen:         # a new run: its rows' prompts, zero counts
            self._pen_reset(st, np.arange(B), pen.prompts, pen.values)
            st["pen_run"] = pen
        if ids is not st["ids"] and ids is not st.get("last_out"):
            # (a stopped row's -1 is no token: any valid id stands in, its row computes nothing that is kept)
            st["ids"][...] = np.maximum(ids.get(), 0) if isinstance(ids, hp.readback_array) else ids
            self._decode_gather(st)
        ns = self._decode_ns(st, top)
        g = False if st["nograph"] else st["graphs"].get((ns, st["sampling"]))
        if g is None and Llama.graph_decode and top + 2 < limit:
            # capture once, as in `_decode_step_hip`: the capture's two real runs store into a scratch history; the
            # positions, the step counter and the ids are put back afterwards
            keep = st["ids"].copy()
            counts = st["counts"].copy() if st["pen"] else None  # (the capture's runs count their fed tokens too)
            scratch = hp.Mailbox(run["hist"].n, (B, 1), unset=run["hist"].unset)
            st["hist_ptr"][...] = np.int64(scratch._ptr)
            lp_restore = self._lp_scratch(st)
            try:
                g = hp.Graph()
                g.capture(lambda: self._decode_launches(st, ns))
                st["graphs"][(ns, st["sampling"])] = g
            except _lib.HipLibraryError as e:
                if e.code != -2:
                    raise
                st["nograph"], g = True, False
            hp.synchronize()
            st["hist_ptr"][...] = np.int64(run["hist"]._ptr)
            lp_restore()
            st["pos"][...] = pos
            st["step"][...] = np.int32(i)
            st["ids"][...] = keep
            if counts is not None:
                st["counts"][...] = counts
            self._decode_gather(st)
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
        st["host_step"] = i + 1
        out = st["last_out"] = run["hist"].slot(i)
        if more and Llama.decode_ahead and (st["graphs"] or st["nograph"]) and top + 1 < limit:
            self._decode_ahead_rows(st, run, i + 1)
        return out if n_lp is None else (out, self._lp_read(st, i))

    def _decode_ahead_rows(self, st, run, i):
        """`_decode_ahead` for a ragged plan: queue step i right behind the one just issued."""
        ns = self._decode_ns(st, int(run["lens"].max()) + i)
        g = False if st["nograph"] else st["graphs"].get((ns, st["sampling"]))
        if g is None:
            return
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
        st["host_step"] = i + 1
        st["ahead"] = ((id(run), i), st["last_out"], run["hist"].slot(i))

    def _decode_step_generic_rows(self, ids, pos, sampling=None, req=None, pen=None, n_lp=None):
        """`_decode_step_generic` with a position per row (pos: host int32, -1 = a stopped row: computed at position 0,
        no cache slot written): k / v are projected into scratch rows and written to each row's own slot, RoPE takes
        each row's own cos / sin row, and the attention runs over each row's own key count (pdn_attention_decode_rows_f32).
        `req` (Llama.serve): the counter id of each row, drawn by the slot tick (default: the row).  `pen`
        (llm/penalties.Rows): the statement of the penalties on the host counts.  Returns the ids of every row, (B, 1)
        int64 (`n_lp`: and the rows' Logprobs, none for rows at -1)."""
        from .. import hipnp as hp, _lib
        L, st = _lib.lib(), hp.stream()
        D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        hd, half = D // H, D // H // 2
        B = ids.shape[0]
        p = np.maximum(pos, 0)
        ws = getattr(self, "_decode_ws_rows", None)
        if ws is None or ws["x"].device_index != hp._state["device"] or ws["x"].shape[0] != B:
            ws = {n: hp.empty((B, w), np.float32) for n, w in
                  (("x", D), ("h", D), ("q", D), ("k", D), ("v", D), ("att", D), ("g", F), ("u", F), ("sw", F),
                   ("logits", V))}
            ws["lens"] = hp.zeros((B,), np.int32)
            self._decode_ws_rows = ws
        ws["lens"][...] = (p + 1).astype(np.int32)
        x, h, q, k, v, att, g, u, sw, logits = (ws[n]._ptr for n in ("x", "h", "q", "k", "v", "att", "g", "u", "sw", "logits"))

        def gemv(a_ptr, K, w, c_ptr, N, beta=0.0, bias=None):
            wd = w.data
            L.call("pdn_gemm_f32", B, N, K, 1.0, a_ptr, K, 1, wd._ptr, wd._strides[0], wd._strides[1], beta, c_ptr,
                   N, bias, 1, 1, 0, 0, 0, 0, 0, 0, None, None, 0, None, 0, st)

        emb = self.tok_embedding.weight.data
        idc = ids if ids.is_contiguous() else ids.copy()
        if pos.min() < 0:                                                 # (a stopped row's -1 is no token)
            idc = hp.asarray(np.maximum(idc.get(), 0))
        L.call("pdn_embedding_gather_f32", emb._ptr, V, D, emb._strides[0], idc._ptr, B, x, hp.err_flag_ptr(), st)
        cos, sin = self.freqs_cos.data._ptr, self.freqs_sin.data._ptr
        for layer in self.layers:
            a, f = layer.attention, layer.ffn
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
            gemv(att, D, a.O.weight, x, D, beta=1.0)                      # x += att @ Wo
            L.call("pdn_rmsnorm_fwd_f32", x, layer.post_attn_norm.weight.data._ptr, h, None, B, D,
                   layer.post_attn_norm.eps, st)
            gemv(h, D, f.gate.weight, g, F)
            gemv(h, D, f.up.weight, u, F)
            L.call("pdn_swiglu_fwd_f32", g, u, sw, B * F, st)
            gemv(sw, F, f.down.weight, x, D, beta=1.0)                    # x += swiglu @ Wdown
        L.call("pdn_rmsnorm_fwd_f32", x, self.norm.weight.data._ptr, h, None, B, D, self.norm.eps, st)
        gemv(h, D, self.lm_head.weight, logits, V,
             bias=self.lm_head.bias.data._ptr if getattr(self.lm_head, "bias", None) is not None else None)
        if pen is not None:
            pen.feed(idc.get(), pos)
            ws["logits"][...] = pen.apply(ws["logits"].get())
        if sampling is None:
            out = ws["logits"].argmax(-1, keepdims=True)
        else:
            out = hp.empty((B, 1), np.int64)          # (counter (pos[b], b): the per-row tick on scratch copies)
            pd, step = hp.asarray(p.astype(np.int32)), hp.zeros((1,), np.int32)
            if req is not None:                       # (counter (pos[b], req[b]): the slot tick, a budget of one token)
                rq, left = hp.asarray(np.asarray(req, np.int32).reshape(B)), hp.asarray(np.ones(B, np.int32))
                L.call("pdn_decode_sample_tick_slots_f32", logits, V, B, V, params_buffer(*sampling)._ptr, out._ptr,
                       pd._ptr, step._ptr, rq._ptr, left._ptr, 1, None, None, None, 0, 0, None, st)
            else:
                L.call("pdn_decode_sample_tick_rows_f32", logits, V, B, V, params_buffer(*sampling)._ptr, out._ptr,
                       pd._ptr, step._ptr, None, None, None, 0, 0, None, st)
        if n_lp is None:
            return out
        tok = np.array(out.get()).reshape(-1)
        tok[pos < 0] = -1
        return out, self._logprobs_rows(ws["logits"], tok, n_lp)

    # -- continuous batching (serve): a finished row takes the next waiting request -------------------------------
    def serve(self, prompts, max_new_tokens, slots=None, temperature=0.0, top_k=0, top_p=1.0, seed=0, stop_ids=(),
              prefill_chunk=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logprobs=None,
              prefix_cache=False):
        """Continuous batching: N requests (`prompts`, N may exceed max_batch_size) through `slots` decode rows
        (default min(N, max_batch_size)).  A row frees when its request yields a stop id or uses up its budget
        (`max_new_tokens`: one int, or one per request; 0 = the request yields nothing and never takes a row).  Before
        the next step the freed rows are refilled -- the lowest free row takes the lowest waiting request -- by one
        batched prompt pass, while the other rows go on decoding.
        Yields, per step, two (slots,) int64 arrays (requests, tokens): the request in row b (-1: empty) and the token it
        produced at this step (the prompt pass's token for a row admitted at this step; -1: none).
        Request r's tokens are the first budget_r tokens of row r of `generate_ragged(prompts, max(budgets), ...)`,
        cut after its first stop id: a sampled token of request r at position t is drawn with Philox counter (t, r),
        whichever row it runs in.  Every argument is checked here (ValueError), before anything runs.
        `prefill_chunk` = C (chunked prefill, the schedule of llm/chunked.py): no prompt pass stalls the other rows;
        every step feeds at most C prompt tokens in total to the rows still prefilling, in request order, and a row yields
        -1 until the step that feeds its last prompt token, which yields its first token.  The tokens of each request are
        those of `serve`; only the step at which they appear changes.  slots + C <= 256.
        `repetition_penalty` / `presence_penalty` / `frequency_penalty` (llm/penalties.py): one set of values for every
        request; each request has its own prompt set and counts -- a row that takes a request starts from its prompt and
        zero counts -- so the promise above holds with penalties too.
        `logprobs` = n (llm/logprobs.py): every step yields (reqs, toks, lp), lp of (slots,) / (slots, n) arrays; a slot
        that yields no token has nan / -1 / nan.
        `prefix_cache` = True or k >= 1 (True = 1; needs `prefill_chunk`; llm/prefix.py): a request whose prompt starts
        with at least k tokens that a cache row still holds from an earlier prompt (its own row's previous request, or
        another row's, live or not) is not fed those tokens: its row takes them -- one pdn_kv_copy_prefix_rows_f32 per
        step for all rows that take from another row, none for a row's own contents -- and its prefill starts behind
        them.  The last prompt token is always fed.  The tokens of each request are those of `serve` without the cache;
        only the step at which they appear changes.  Only the graph path with the mixed step reuses anything: on every
        other path (a library without the mixed step, more than 8 key ranges, wide_decode off, the generic rows, the
        `cpu` device) a prompt completes with one whole pass from position 0, so every prompt is computed in full and
        steps and tokens are exactly those without the cache.  `self.prefix_stats` holds the run's figures (requests,
        hits, prompt_tokens, reused_tokens, copies, launches) as it goes; with the cache off it is left alone."""
        temperature, top_k, top_p, seed = check_sampling_args(temperature, top_k, top_p, seed)
        penalty = pen_np.check_args(repetition_penalty, presence_penalty, frequency_penalty)
        n_lp = lp_np.check_n(logprobs)
        k_pre = prefix_np.check_arg(prefix_cache, prefill_chunk)
        V = self.vocab_size
        rows = [np.asarray(p.numpy() if isinstance(p, Tensor) else p).reshape(-1) for p in prompts]
        if not rows:
            raise ValueError("serve needs at least one prompt")
        N = len(rows)
        budgets = [max_new_tokens] * N if np.ndim(max_new_tokens) == 0 else list(max_new_tokens)
        if len(budgets) != N:
            raise ValueError(f"max_new_tokens: {len(budgets)} budgets for {N} prompts")
        for r, n in enumerate(budgets):
            if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer, float, np.floating)) \
                    or int(n) != n or n < 0:
                raise ValueError(f"max_new_tokens of request {r} must be a non-negative integer, got {n!r}")
        budgets = np.array([int(n) for n in budgets], np.int64)
        cache = self.layers[0].attention.cache_k
        if slots is None:
            slots = min(N, cache.shape[0])
        if isinstance(slots, (bool, np.bool_)) or int(slots) != slots or not 1 <= slots <= cache.shape[0]:
            raise ValueError(f"slots must be an integer in [1, {cache.shape[0]}] (the KV cache's max_batch_size), "
                             f"got {slots!r}")
        limit = min(cache.shape[1], self.freqs_cos.shape[0])     # positions the cache / RoPE table hold
        for r, (p, n) in enumerate(zip(rows, budgets)):
            if p.size == 0:
                raise ValueError(f"prompt {r} is empty")
            if p.dtype.kind not in "iu" or p.min() < 0 or p.max() >= V:
                raise ValueError(f"prompt {r}: token ids must be integers in [0, {V})")
            last = p.size + n - 1                                 # (the position of the request's last decode step)
            if n > 0 and (p.size > cache.shape[1] or (n > 1 and last >= limit)):
                raise ValueError(f"prompt {r}: its last position {last} is outside the KV cache / RoPE table "
                                 f"(max_seq_len {cache.shape[1]}, {self.freqs_cos.shape[0]} RoPE rows)")
        stops = np.asarray(sorted({int(t) for t in stop_ids}), np.int64)
        if stops.size and (stops.min() < 0 or stops.max() >= V):
            raise ValueError(f"stop ids must lie in [0, {V}), got {stops.tolist()}")
        sampling = (temperature, top_k, top_p, seed) if temperature > 0 else None
        C = chunked.check_chunk(prefill_chunk, slots)
        if C is not None:
            return self._serve_chunked([p.astype(np.int64) for p in rows], budgets, int(slots), C, sampling, stops,
                                       penalty, n_lp, k_pre)
        return self._serve([p.astype(np.int64) for p in rows], budgets, int(slots), sampling, stops, penalty, n_lp)

    def serve_all(self, prompts, max_new_tokens, slots=None, temperature=0.0, top_k=0, top_p=1.0, seed=0, stop_ids=(),
                  prefill_chunk=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                  logprobs=None, prefix_cache=False):
        """`serve` run to the end: a list of N int64 arrays, request r's generated tokens in order.  `logprobs` = n: a
        list of (tokens, Logprobs) instead, the arrays of length k / (k, n) for a request's k tokens."""
        it = self.serve(prompts, max_new_tokens, slots, temperature, top_k, top_p, seed, stop_ids, prefill_chunk,
                        repetition_penalty, presence_penalty, frequency_penalty, logprobs, prefix_cache)
        out = [[] for _ in range(len(prompts))]
        lps = [[] for _ in range(len(prompts))]
        for step in it:
            reqs, toks = step[0], step[1]
            for b, (r, t) in enumerate(zip(reqs, toks)):
                if r >= 0 and t >= 0:
                    out[r].append(int(t))
                    if logprobs is not None:
                        lps[r].append((step[2].token[b], step[2].top_ids[b], step[2].top_logprobs[b]))
        if logprobs is None:
            return [np.array(o, np.int64) for o in out]
        n = int(logprobs)
        # (reshape to (k, n) by count: with n = 0 or k = 0 a -1 could not be inferred)
        return [(np.array(o, np.int64), lp_np.Logprobs(np.array([e[0] for e in l], np.float32).reshape(len(l)),
                                                       np.array([e[1] for e in l], np.int64).reshape(len(l), n),
                                                       np.array([e[2] for e in l], np.float32).reshape(len(l), n)))
                for o, l in zip(out, lps)]

    def _serve(self, rows, budgets, S, sampling, stops, penalty=None, n_lp=None):
        """The scheduler of `serve`.  Per step: the rows holding a request decode one token, then the rows freed by the
        previous step take the waiting requests in order through one prompt pass (`_serve_prefill`), then the step is
        yielded.  The host keeps, per row, the request, the position of its next decode step, the tokens it may still
        produce and its last token; on the graph path the device keeps the same in the served plan (`_serve_begin`) and
        the host writes it only after an admission, when every queued step has been read."""
        lens = np.array([r.size for r in rows], np.int64)
        queue = [r for r in range(len(rows)) if budgets[r] > 0]   # FIFO by index; a budget of 0 never takes a row
        req = np.full(S, -1, np.int64)
        pos = np.full(S, -1, np.int64)
        left = np.zeros(S, np.int64)
        last = np.zeros(S, np.int64)
        dev = self.tok_embedding.weight.device
        hip = (Llama.fast_decode and dev.is_hip and not self._train
               and self.lm_head.weight.dtype == np.float32 and (self.embed_dim // self.n_heads) % 4 == 0)
        st = self._serve_begin(S, sampling, stops, penalty, n_lp) if hip else None   # None: the plan refuses -> generic
        pen = None if penalty is None or st is not None else pen_np.Rows(S, self.vocab_size, penalty)   # (host counts)
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
                    ids, rq = last.reshape(S, 1), np.maximum(req, 0)
                    if hip:
                        from .. import hipnp as hp
                        out = self._decode_step_generic_rows(hp.asarray(ids), p.astype(np.int32), sampling, rq,
                                                             pen=pen, n_lp=n_lp)
                    else:
                        out = self._step_module_rows(Tensor(ids, dtype=np.int64, device=dev), p, sampling, rq,
                                                     pen=pen, n_lp=n_lp)
                    if n_lp is not None:
                        out, lpr = out
                        lp_np.merge(lpv, np.flatnonzero(run), lp_np.Logprobs(*(a[run] for a in lpr)))
                    out = out.get() if hip else out.numpy()
                    toks[run] = out.reshape(-1)[run]
                shown = req.copy()
                if adm.size:
                    first = self._serve_prefill([rows[r] for r in new], adm, new, sampling, penalty, n_lp)
                    if n_lp is not None:
                        first, lpf = first
                        lp_np.merge(lpv, adm, lpf)
                    if pen is not None:
                        pen.reset(adm, [rows[r] for r in new])
                    if st is not None and st["pending"]:
                        d = self._serve_read(st, lpv, run)       # (stream order: that step ran before the prefill)
                        toks[run] = d[run]
                    toks[adm], shown[adm] = first, new
                    req[adm], pos[adm], left[adm] = new, lens[new], budgets[new]
                # every row that produced a token: one position further, one token less; a request ends at its budget
                # or at a stop id, and its row is free for the next step
                has = shown >= 0
                left[has] -= 1
                pos[has] += 1
                last[has] = toks[has]
                done = has & ((left <= 0) | np.isin(toks, stops))
                req[done], pos[done], left[done] = -1, -1, 0
                if st is not None and adm.size:
                    self._serve_write(st, req, pos, left, last)
                    if st["pen"]:                                # (no step queued: after every step of the old request)
                        self._pen_reset(st, adm, [rows[r] for r in new], penalty)
                    if (req >= 0).any():
                        self._serve_ahead(st, int(np.where(req >= 0, pos, -1).max()))
                yield (shown, toks) if n_lp is None else (shown, toks, lpv)
        finally:
            if st is not None and st["pending"]:
                from .. import hipnp as hp
                hp.synchronize()                                 # (queued steps store into this run's history)
                st["pending"] = 0

    def _serve_prefill(self, prompts, rows, reqs, sampling, penalty=None, n_lp=None):
        """Admit requests `reqs` (their prompts) into decode rows `rows`: the prompts right-padded to the longest run as one
        batched causal pass from position 0 into a staging cache (the layers' caches point at it meanwhile), then
        pdn_kv_store_slots_f32 puts prompt i's keys / values, positions [0, len_i), into cache row rows[i] and zeroes
        position len_i there -- the slot a decode step attends to but never writes (`generate`'s step at position p feeds
        the token of position p - 1), which in a fresh cache holds zeros.  No pad position and no other row is written.
        `penalty`: the logits penalised for each prompt first.  Returns the first token of each request (counter (len_i,
        reqs[i]) when sampled), host int64 (`n_lp`: and their Logprobs)."""
        logits = self._prefill_rows(prompts, rows)
        if penalty is not None:
            logits = self._penalize_prompt(logits, prompts, penalty)
        lens = np.array([p.size for p in prompts], np.int64)
        first = logits.argmax(-1, True) if sampling is None else sample_next_rows(logits, lens, *sampling, rows=reqs)
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
    def _serve_begin(self, S, sampling, stops, penalty=None, n_lp=None):
        from .. import hipnp as hp
        st = self._decode_plan(S, sampling is not None, ragged=True, serve=True, penalty=penalty is not None, n_lp=n_lp)
        if st is None:
            return None
        if st["pending"]:
            hp.synchronize()                                     # (an abandoned run's queued steps)
        mask = np.zeros(-(-self.vocab_size // 32), np.uint32)
        np.bitwise_or.at(mask, stops >> 5, np.uint32(1) << (stops & 31).astype(np.uint32))
        st["hist"] = hp.Mailbox(st["ring"], (S, 1), unset=np.iinfo(np.int64).min)
        st["hist_ptr"][...] = np.int64(st["hist"]._ptr)
        self._lp_begin(st)
        st["stop"][...] = mask.view(np.int32)
        st["pos"][...] = np.full(S, -1, np.int32)
        st["step"][...] = np.int32(0)
        st["left"][...] = np.zeros(S, np.int32)
        st["req"][...] = np.zeros(S, np.int32)
        if sampling is not None and st["params_val"] != sampling:
            st["params"][...] = params_bytes(*sampling)
        st["params_val"] = sampling
        if penalty is not None:                                  # (every row is reset when it takes a request)
            self._pen_reset(st, [], [], penalty)
        st["pending"], st["read"] = 0, 0
        return st

    def _serve_issue(self, st, top):
        """Issue the next decode step of a served plan (its furthest row at position `top`); captures its graph first
        when this range count has none -- the capture's two real runs store into a scratch history and the rows' state
        is put back afterwards."""
        from .. import hipnp as hp, _lib
        if self._decode_st is not st:
            raise RuntimeError("another generation replaced the plan of a running serve() on this model")
        ns = self._decode_ns(st, top)
        g = False if st["nograph"] else st["graphs"].get((ns, st["sampling"]))
        if g is None and Llama.graph_decode:
            # (penalty plans: the capture's runs count their fed tokens too -- the counts are put back as well)
            keep = {n: st[n].copy() for n in ("ids", "pos", "step", "left") + (("counts",) if st["pen"] else ())}
            scratch = hp.Mailbox(st["ring"], (st["B"], 1), unset=st["hist"].unset)
            st["hist_ptr"][...] = np.int64(scratch._ptr)
            lp_restore = self._lp_scratch(st)
            try:
                g = hp.Graph()
                g.capture(lambda: self._decode_launches(st, ns))
                st["graphs"][(ns, st["sampling"])] = g
            except _lib.HipLibraryError as e:
                if e.code != -2:                                 # PDN_EUNSUPPORTED: no graph support (emulated ABI)
                    raise
                st["nograph"], g = True, False
            hp.synchronize()
            st["hist_ptr"][...] = np.int64(st["hist"]._ptr)
            lp_restore()
            for n, v in keep.items():
                st[n][...] = v
            self._decode_gather(st)
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
        st["pending"] += 1

    def _serve_ahead(self, st, top):
        """Queue the next step right behind the issued ones (decode_ahead), if its graph exists: a row that ends in the
        step before computes nothing that is kept (its position is -1 on the device by then)."""
        if not Llama.decode_ahead or not (st["graphs"] or st["nograph"]):
            return
        ns = self._decode_ns(st, top)
        g = False if st["nograph"] else st["graphs"].get((ns, st["sampling"]))
        if g is None:
            return                                               # (a new range count: captured when next issued)
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
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
        ids, budgets and last tokens -- written in stream order, and x = the embedding rows of those tokens."""
        st["pos"][...] = pos.astype(np.int32)
        st["req"][...] = np.maximum(req, 0).astype(np.int32)
        st["left"][...] = left.astype(np.int32)
        st["ids"][...] = last.reshape(-1, 1)
        self._decode_gather(st)

    # -- chunked prefill (serve(prefill_chunk=C)): prompts fed C tokens per step (statement: llm/chunked.py) -----------
    def _serve_chunked(self, rows, budgets, S, C, sampling, stops, penalty=None, n_lp=None, prefix=None):
        """The scheduler of `serve` with a chunk: llm/chunked.Schedule decides, per step, which rows decode and which
        prompt tokens are fed.  Graph path (`_mixed_begin`): a step with prompt tokens runs the mixed step (the decode
        rows and the chunks as query rows of the wide product, csrc/extend.hip), a step without runs the served step.
        Every other path decodes as `_serve` does, and a prompt pass runs when the schedule completes prompts: one
        `_serve_prefill` for the requests whose prompts complete in that step.
        `prefix` = k (the prefix cache, llm/prefix.Schedule): on the graph path the rows admitted in a step that reuse
        another row's tokens take them through one copy launch, issued eagerly before the step (`_prefix_copy`), and
        their prefill starts at fed = n; every other path starts every prompt at 0 (the schedule with reuse forced off)."""
        lens = np.array([r.size for r in rows], np.int64)
        dev = self.tok_embedding.weight.device
        hip = (Llama.fast_decode and dev.is_hip and not self._train
               and self.lm_head.weight.dtype == np.float32 and (self.embed_dim // self.n_heads) % 4 == 0)
        st = self._mixed_begin(S, C, sampling, stops, penalty, n_lp) if hip else None
        if prefix is None:
            sch = chunked.Schedule(lens, budgets, S, C)
        else:
            sch = prefix_np.Schedule(rows, budgets, S, C, prefix if st is not None else None)
            self.prefix_stats = sch.stats
            if st is not None:
                st.pop("prefix", None)                          # (the cache pointer table: built by the run's first copy)
        pen = None if penalty is None or st is not None else pen_np.Rows(S, self.vocab_size, penalty)   # (host counts)
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
                        p, rq = np.where(dec, sch.pos, -1), np.maximum(sch.req, 0)
                        ids = sch.last.reshape(S, 1)
                        if hip:
                            from .. import hipnp as hp
                            out = self._decode_step_generic_rows(hp.asarray(ids), p.astype(np.int32), sampling, rq,
                                                                 pen=pen, n_lp=n_lp)
                        else:
                            out = self._step_module_rows(Tensor(ids, dtype=np.int64, device=dev), p, sampling, rq,
                                                         pen=pen, n_lp=n_lp)
                        if n_lp is not None:
                            out, lpr = out
                            lp_np.merge(lpv, np.flatnonzero(dec), lp_np.Logprobs(*(a[dec] for a in lpr)))
                        out = out.get() if hip else out.numpy()
                        toks[dec] = out.reshape(-1)[dec]
                    if comp.any():
                        b = np.flatnonzero(comp)
                        first = self._serve_prefill([rows[r] for r in sch.req[b]], b, sch.req[b], sampling, penalty,
                                                    n_lp)
                        if n_lp is not None:
                            first, lpf = first
                            lp_np.merge(lpv, b, lpf)
                        toks[b] = first
                shown = sch.finish(n, toks, stops)
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
        return bool(Llama.wide_decode and S + C <= 256 and all(_lib.provides(n) for n in _MIXED_ENTRIES)
                    and L.query("pdn_decode_mixed_supported", D, H, D // H, F, V, cache_len))

    def _mixed_begin(self, S, C, sampling, stops, penalty=None, n_lp=None):
        """The served plan (`_serve_begin`) plus the buffers of the mixed step (`mixed`), or None when either refuses."""
        from .. import hipnp as hp, _lib
        if not self._mixed_ok(S, C):
            return None
        st = self._serve_begin(S, sampling, stops, penalty, n_lp)
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
        st["left"][...] = np.where(inc | comp, sch.left, 0).astype(np.int32)
        M["qpos"][...] = qpos
        M["runs"][...] = runs
        M["tok"][...] = tok
        M["emit"][...] = emit

    def _mixed_issue(self, st, sch, n, inc, comp, rows):
        """Issue one mixed step (no step queued): upload its layout, capture its graph first when there is none."""
        from .. import hipnp as hp, _lib
        if self._decode_st is not st:
            raise RuntimeError("another generation replaced the plan of a running serve() on this model")
        self._mixed_layout(st, sch, n, inc, comp, rows)
        ns = st["ns"]
        gk = (ns, st["sampling"], "mixed", st["mixed"]["C"])
        g = False if st["nograph"] else st["graphs"].get(gk)
        if g is None and Llama.graph_decode:
            keep = {n: st[n].copy() for n in ("ids", "pos", "step", "left") + (("counts",) if st["pen"] else ())}
            scratch = hp.Mailbox(st["ring"], (st["B"], 1), unset=st["hist"].unset)
            st["hist_ptr"][...] = np.int64(scratch._ptr)
            lp_restore = self._lp_scratch(st)
            try:
                g = hp.Graph()
                g.capture(lambda: self._mixed_launches(st, ns))
                st["graphs"][gk] = g
            except _lib.HipLibraryError as e:
                if e.code != -2:                                 # PDN_EUNSUPPORTED: no graph support (emulated ABI)
                    raise
                st["nograph"], g = True, False
            hp.synchronize()
            st["hist_ptr"][...] = np.int64(st["hist"]._ptr)
            lp_restore()
            for k, v in keep.items():
                st[k][...] = v
            self._decode_gather(st)
        if g:
            g.replay()
        else:
            self._mixed_launches(st, ns)
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
        head = self.lm_head
        bias = head.bias.data._ptr if getattr(head, "bias", None) is not None else None
        full = st["sampling"] or st["pen"]
        cv, ci = (None, None) if full else (M["cand_v"]._ptr, M["cand_i"]._ptr)
        L.call("pdn_decode_wide_gemm_f32", xe, D, 1, self.norm.weight.data._ptr, self.norm.eps, 0, 0,
               head.weight.data._ptr, V, V, 0, bias, st["logits"]._ptr, V, 0 if full else 2, cv, ci, st["pos"]._ptr, S,
               D, V, work, s)
        # (penalty plans: a row completing its prompt here is at position len = start and counts nothing; greedy: the
        #  plan's candidates are those of the penalty kernel)
        self._pen_step(st, s)
        cands = st if st["pen"] else M
        cnt = (st["pos"]._ptr, st["step"]._ptr, M["arrive"]._ptr)
        out = (st["hist_ptr"]._ptr, emb._ptr, emb._strides[0], D, st["x"]._ptr, s)
        if st["sampling"]:
            L.call("pdn_decode_wide_sample_tick_slots_f32", st["logits"]._ptr, V, S, V, st["params"]._ptr,
                   st["ids"]._ptr, *cnt, st["req"]._ptr, st["left"]._ptr, st["ring"], st["stop"]._ptr, *out)
        else:
            L.call("pdn_decode_wide_pick_tick_slots_f32", cands["cand_v"]._ptr, cands["cand_i"]._ptr, S,
                   cands["cand_v"].shape[1], st["ids"]._ptr, *cnt, st["req"]._ptr, st["left"]._ptr, st["ring"],
                   st["stop"]._ptr, *out)
        self._lp_tick(st, s)

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
        hip = (Llama.fast_decode and dev.is_hip and not self._train
               and self.lm_head.weight.dtype == np.float32 and (self.embed_dim // self.n_heads) % 4 == 0)
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
        return bool(Llama.wide_decode and B * (k + 1) <= 256 and all(_lib.provides(n) for n in _SPEC_ENTRIES)
                    and L.query("pdn_decode_mixed_supported", D, H, D // H, F, V, cache_len))

    def _spec_begin(self, R, k, sampling):
        """The plan of the speculative pass (buffers, weight views, its graph), kept across calls while the model's arrays
        and (B, k, sampling) stay; then this run's row state uploaded.  None when the library or the model's layout
        refuses it."""
        from .. import hipnp as hp, _lib
        B = len(R.out)
        if not self._spec_ok(B, k):
            return None
        D, H, F, V = self.embed_dim, self.n_heads, self.ffn_dim, self.vocab_size
        cache_len = self.layers[0].attention.cache_k.shape[1]
        ns = int(os.environ.get("PDN_DECODE_SPLITS", "0")) or (1 if cache_len <= 256 else 4)
        if ns > 8:
            return None
        key = (B, k, bool(sampling), hp._state["device"], ns, cache_len, tuple(self._weight_ptrs()))
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
                  "pending": 0, "sampling": bool(sampling), "params_val": None,
                  "work": hp.zeros((max(work, 4),), np.float32),
                  "cand_v": hp.empty((Rq, nblk), np.float32), "cand_i": hp.empty((Rq, nblk), np.int32),
                  "logits": hp.empty((Rq, V), np.float32), "params": hp.zeros((3,), np.int64),
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
        mask = np.zeros(-(-V // 32), np.uint32)
        np.bitwise_or.at(mask, R.stops >> 5, np.uint32(1) << (R.stops & 31).astype(np.uint32))
        st["hist"][...] = hist
        st["hlen"][...] = np.array([h.size for h in R.hist], np.int32)
        st["pos"][...] = R.pos.astype(np.int32)
        st["left"][...] = R.left.astype(np.int32)
        st["step"][...] = np.int32(0)
        st["stop"][...] = mask.view(np.int32)
        # one mailbox slot per pass: a pass moves every live row at least one token on, so n - 1 passes finish the run
        st["mbox"] = hp.Mailbox(max(int(R.left.max()), 1), (B, k + 4), unset=np.iinfo(np.int64).min)
        st["mbox_ptr"][...] = np.int64(st["mbox"]._ptr)
        if st["params_val"] != sampling:
            if sampling is not None:
                st["params"][...] = params_bytes(*sampling)
            st["params_val"] = sampling
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
        head = self.lm_head
        bias = head.bias.data._ptr if getattr(head, "bias", None) is not None else None
        full = st["sampling"]
        cv, ci = (None, None) if full else (p["cand_v"], p["cand_i"])
        L.call("pdn_decode_wide_gemm_f32", p["x"], D, 1, self.norm.weight.data._ptr, self.norm.eps, 0, 0,
               head.weight.data._ptr, V, V, 0, bias, p["logits"], V, 0 if full else 2, cv, ci, p["qpos"], Rq, D, V,
               p["work"], s)
        row = (p["tok"], p["qpos"], B, k, p["picks"], p["hist"], st["hw"], p["hlen"], p["pos"], p["left"], p["stop"],
               p["step"], p["mbox_ptr"], s)
        if full:
            L.call("pdn_spec_verify_sample_tick_f32", p["logits"], V, V, st["params"]._ptr, *row)
        else:
            L.call("pdn_spec_verify_pick_tick_f32", p["cand_v"], p["cand_i"], st["cand_v"].shape[1], *row)

    def _spec_issue(self, st):
        """Queue one target pass; the first one of a plan captures its graph (whose two real runs work on a copy of the
        row state and a scratch mailbox: the state is put back afterwards)."""
        from .. import hipnp as hp, _lib
        g = False if st["nograph"] else st["graph"]
        if g is None and Llama.graph_decode:
            keep = {n: st[n].copy() for n in ("hist", "hlen", "pos", "left", "step")}
            scratch = hp.Mailbox(2, (st["B"], st["k"] + 4), unset=np.iinfo(np.int64).min)
            st["mbox_ptr"][...] = np.int64(scratch._ptr)
            try:
                g = hp.Graph()
                g.capture(lambda: self._spec_launches(st))
                st["graph"] = g
            except _lib.HipLibraryError as e:
                if e.code != -2:                                 # PDN_EUNSUPPORTED: no graph support (emulated ABI)
                    raise
                st["nograph"], g = True, False
            hp.synchronize()
            st["mbox_ptr"][...] = np.int64(st["mbox"]._ptr)
            for n, v in keep.items():
                st[n][...] = v
        if g:
            g.replay()
        else:
            self._spec_launches(st)
        st["pending"] += 1

    def _spec_device(self, st, R):
        """The device path: passes queued back to back (one ahead of the one being read when `decode_ahead`), each read
        from its mailbox slot [count, drafted, accepted, tokens...] per row.  A pass is queued only while some live row
        may still need it: its budget exceeds the passes already queued for it."""
        from .. import hipnp as hp
        B, k = st["B"], st["k"]
        try:
            while True:
                depth = 2 if Llama.decode_ahead else 1
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

    # -- beam search: the W most probable continuations of each prompt (statement: llm/beam.py) ----------------------
    def beam_search(self, prompts, max_new_tokens, num_beams, length_penalty=1.0, stop_ids=()):
        """Beam search over B prompts (ragged lengths allowed) with `num_beams` = W beams each: rows g * W .. g * W + W - 1
        of the KV cache hold prompt g's beams.  Returns a list of B lists of W (tokens: int64 array, score: float) pairs,
        best first: the W best hypotheses of each prompt by score / n_gen ** length_penalty (llm/beam.py states the rules).
        A hypothesis ends at a stop id (included) or after `max_new_tokens` tokens; a prompt is done once it holds W
        hypotheses ended by a stop id.  Every argument is checked here (ValueError), before anything runs."""
        V = self.vocab_size
        if isinstance(num_beams, (bool, np.bool_)) or int(num_beams) != num_beams or not 1 <= num_beams <= beam_np.MAX_BEAMS:
            raise ValueError(f"num_beams must be an integer in [1, {beam_np.MAX_BEAMS}], got {num_beams!r}")
        W = int(num_beams)
        if isinstance(max_new_tokens, (bool, np.bool_)) or int(max_new_tokens) != max_new_tokens or max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be a positive integer, got {max_new_tokens!r}")
        n = int(max_new_tokens)
        length_penalty = float(length_penalty)
        if not np.isfinite(length_penalty):
            raise ValueError(f"length_penalty must be finite, got {length_penalty}")
        rows = [np.asarray(p.numpy() if isinstance(p, Tensor) else p).reshape(-1) for p in prompts]
        if not rows:
            raise ValueError("beam_search needs at least one prompt")
        cache = self.layers[0].attention.cache_k
        B = len(rows) * W
        if B > cache.shape[0] or B > 256:
            raise ValueError(f"{len(rows)} prompts x {W} beams = {B} rows exceed the KV cache's max_batch_size "
                             f"{cache.shape[0]} or 256")
        limit = min(cache.shape[1], self.freqs_cos.shape[0])
        for g, r in enumerate(rows):
            if r.size == 0:
                raise ValueError(f"prompt {g} is empty")
            if r.dtype.kind not in "iu" or r.min() < 0 or r.max() >= V:
                raise ValueError(f"prompt {g}: token ids must be integers in [0, {V})")
            last = r.size + n - 1
            if r.size > cache.shape[1] or (n > 1 and last >= limit):
                raise ValueError(f"prompt {g}: its last position {last} is outside the KV cache / RoPE table "
                                 f"(max_seq_len {cache.shape[1]}, {self.freqs_cos.shape[0]} RoPE rows)")
        stops = np.asarray(sorted({int(t) for t in stop_ids}), np.int64)
        if stops.size and (stops.min() < 0 or stops.max() >= V):
            raise ValueError(f"stop ids must lie in [0, {V}), got {stops.tolist()}")
        if stops.size > beam_np.MAX_STOPS:
            raise ValueError(f"at most {beam_np.MAX_STOPS} distinct stop ids, got {stops.size}")
        if V - stops.size < W:
            raise ValueError(f"{V} tokens minus {stops.size} stop ids leave fewer than num_beams = {W}")
        rows = [r.astype(np.int64) for r in rows]
        dev = self.tok_embedding.weight.device
        if (Llama.fast_decode and dev.is_hip and not self._train and self.lm_head.weight.dtype == np.float32
                and (self.embed_dim // self.n_heads) % 4 == 0):
            out = self._beam_device(rows, n, W, length_penalty, stops)
        else:
            out = self._beam_module(rows, n, W, length_penalty, stops)
        # the rows' caches back to zeros, as a fresh model holds them: a later generation reads the slot after its prompt
        # before writing it (the reference's decode positions), so nothing of this search may stay there
        T = min(cache.shape[1], max(r.size for r in rows) + n + 1)
        for c in (c for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)):
            c.data[:B, :T] = 0
        return out

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
        written -- and the rows' state is put back afterwards."""
        from .. import hipnp as hp, _lib
        ns = self._decode_ns(st, top)
        g = False if st["nograph"] else st["graphs"].get((ns, "beam"))
        if g is None and Llama.graph_decode:
            keep = {n: st[n].copy() for n in ("ids", "pos", "step")}
            k = int(keep["step"].get()[0])
            st["pos"][...] = np.int32(-1)
            try:
                g = hp.Graph()
                g.capture(lambda: self._decode_launches(st, ns))
                st["graphs"][(ns, "beam")] = g
            except _lib.HipLibraryError as e:
                if e.code != -2:                                 # PDN_EUNSUPPORTED: no graph support (emulated ABI)
                    raise
                st["nograph"], g = True, False
            hp.synchronize()
            live = st["bm"]["live"]
            live.host[k:min(k + 2, live.n)] = live.unset         # (the capture's runs counted no live group there)
            for n_, v in keep.items():
                st[n_][...] = v
            self._decode_gather(st)
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)

    def _beam_ahead(self, st, top):
        """Queue the next beam step right behind the issued one if its graph exists (decode_ahead); True if queued."""
        if not Llama.decode_ahead:
            return False
        ns = self._decode_ns(st, top)
        g = False if st["nograph"] else st["graphs"].get((ns, "beam"))
        if g is None:
            return False
        if g:
            g.replay()
        else:
            self._decode_launches(st, ns)
        return True
