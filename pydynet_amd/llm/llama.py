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
tape altogether (`_decode_step_hip`, llm/decode_steps.py).

This module holds the model, its training entries and the public generation entry points with their argument checks.
The generation engine is four mixins of `Llama`: llm/decode_plan.py (the plan of the graph-replayed step, its launches
and the one capture-or-replay issuer), llm/decode_steps.py (the steps of `generate` / `generate_ragged`, graph, generic
and tape-node), llm/decode_serve.py (`serve`: continuous batching, chunked prefill, prefix cache) and
llm/decode_search.py (speculative decoding, beam search).
"""
import numpy as np

from .. import nn
from ..autograd import is_grad_enable
from ..core import Tensor, fused
from ..special import zeros
from . import beam as beam_np
from . import chunked
from . import logprobs as lp_np
from . import logit_edits as edit_np
from . import penalties as pen_np
from . import prefix as prefix_np
from . import speculative as spec_np
from . import stop_sequences as ss_np
from . import token_fsm as fsm_np
from .decode_plan import DecodePlan
from .decode_search import SearchEngine
from .decode_serve import ServeEngine
from .decode_steps import DecodeSteps
from .sampling import active as active_sampling, check_args as check_sampling_args, check_request_args


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

    def __call__(self, x, start_pos, mask, freqs_cos, freqs_sin, residual=None, segment_ids=None):
        B, L, _ = x.shape
        H, hd = self.n_heads, self.head_dim
        if segment_ids is not None:
            return self._segmented(x, start_pos, mask, freqs_cos, freqs_sin, residual, segment_ids)
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

    def _segmented(self, x, start_pos, mask, freqs_cos, freqs_sin, residual, segment_ids):
        """Packed rows (`segment_ids`: core/fused/segments.py): a query sees the keys of its own document only.  Training
        at start_pos 0 only; the one-node form where its kernels take the shape, else the separate nodes with the same
        mask."""
        B, L, _ = x.shape
        H, hd = self.n_heads, self.head_dim
        if not self._train or start_pos != 0 or mask is None:
            raise ValueError("segment_ids are for training passes over whole rows (train mode, start_pos 0, more than one position)")
        if is_grad_enable() and fused.qkv_attention.applicable(x, L, hd, segment_ids):
            out = fused.qkv_attention(x, self.Q.weight, self.K.weight, self.V.weight, freqs_cos, freqs_sin, H,
                                      segment_ids=segment_ids)
        else:
            xq = self.Q(x).reshape(B, L, H, hd)
            xk = self.K(x).reshape(B, L, H, hd)
            xv = self.V(x).reshape(B, L, H, hd)
            xq, xk = apply_rotary_emb(xq, xk, freqs_cos, freqs_sin)
            out = fused.attention(xq, xk, xv, causal=True, start_pos=0, segment_ids=segment_ids)
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

    def forward(self, x, start_pos, mask, freqs_cos, freqs_sin, segment_ids=None):
        # z = x + attn(norm(x)); out = z + ffn(norm(z)) -- both adds ride in the GEMM epilogues
        if segment_ids is None:
            z = self.attention(self.input_norm(x), start_pos, mask, freqs_cos, freqs_sin, residual=x)
        else:
            z = self.attention(self.input_norm(x), start_pos, mask, freqs_cos, freqs_sin, residual=x, segment_ids=segment_ids)
        return self.ffn(self.post_attn_norm(z), residual=z)

    def step_rows(self, x, pos, freqs_cos, freqs_sin):
        z = self.attention.step_rows(self.input_norm(x), pos, freqs_cos, freqs_sin, residual=x)
        return self.ffn(self.post_attn_norm(z), residual=z)


class Llama(DecodePlan, DecodeSteps, ServeEngine, SearchEngine, nn.Module):
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

    def _forward_hidden(self, input_ids, start_pos: int, segment_ids=None):
        L = input_ids.shape[-1]
        h = self.tok_embedding(input_ids)
        if segment_ids is not None:
            # packed rows: the documents' bounds once per step, shared by every layer (core/fused/segments.py)
            if not self._train or start_pos != 0:
                raise ValueError("segment_ids are for training passes over whole rows (train mode, start_pos 0)")
            segment_ids = fused.segment_bounds(segment_ids, h.device.is_hip)
            if segment_ids.shape != tuple(h.shape[:2]):
                raise ValueError(f"segment_ids of shape {segment_ids.shape} for input_ids of shape {tuple(h.shape[:2])}")
            if L == 1:
                segment_ids = None            # (a single position sees itself)
        cos = self.freqs_cos[start_pos:start_pos + L]
        sin = self.freqs_sin[start_pos:start_pos + L]
        # the reference rebuilds an additive -inf mask on the host every call (model.py:199-203);
        # here causality is a flag of the fused attention node and nothing is uploaded.
        mask = True if L > 1 else None
        # a training pass: the fp16 plane images of all layers' weights in one launch, bound around the layer loop; the
        # backward forms are left on the pass's last node, where Tensor.backward finds them (core/fused/wimages.py)
        fwd_images, bwd_images = self._pass_images(h, L) if start_pos == 0 and mask is not None else (None, None)
        bound = fwd_images is not None and fwd_images.bind()
        try:
            for layer in self.layers:
                h = layer(h, start_pos, mask, cos, sin) if segment_ids is None else \
                    layer(h, start_pos, mask, cos, sin, segment_ids=segment_ids)
        finally:
            if bound:
                fwd_images.release()
        out = self.norm(h)
        if bwd_images is not None and out.requires_grad:
            out._backward_images = bwd_images
        return out

    def _pass_images(self, h, L):
        """(forward, backward) `fused.wimages.ImageSet`s of this training forward over the hidden state `h`, or (None, None)"""
        wim = fused.wimages
        T = h.size // h.shape[-1]
        if not (self._train and is_grad_enable() and h.device.is_hip and h.dtype == np.float32 and T >= wim.min_rows
                and wim.enabled()):
            return None, None
        fwd, bwd, keep = [], [], []
        for layer in self.layers:
            att, ffn = layer.attention, layer.ffn
            ws = [m.weight.data for m in (att.Q, att.K, att.V, att.O, ffn.gate, ffn.up, ffn.down)]
            f, b = wim.layer_forms(*ws, T, L, att.head_dim)
            fwd += f
            bwd += b
            keep += ws
        return (wim.ImageSet(fwd, keep) if fwd else None), (wim.ImageSet(bwd, keep) if bwd else None)

    def forward_logits(self, input_ids, start_pos: int = 0):
        return self.lm_head(self._forward_hidden(input_ids, start_pos))

    def set_trainable_parameters(self, trainable_prefixes=("lm_head",)):
        trainable = frozen = 0
        for name, p in self._parameters.items():
            p.requires_grad = any(name.startswith(pre) for pre in trainable_prefixes)
            trainable, frozen = trainable + p.requires_grad, frozen + (not p.requires_grad)
        return trainable, frozen

    @staticmethod
    def _smoothing(criterion, label_smoothing, z_loss):
        """(label_smoothing, z_loss) from the keywords, or from a criterion that carries them -- not from both"""
        if criterion is not None and (label_smoothing != 0.0 or z_loss != 0.0):
            raise ValueError("pass label_smoothing / z_loss through the criterion (nn.CrossEntropyLoss(label_smoothing=..., "
                             "z_loss=...)), not beside it")
        if criterion is not None:
            label_smoothing, z_loss = getattr(criterion, "label_smoothing", 0.0), getattr(criterion, "z_loss", 0.0)
        return fused.smooth_loss.check_arguments(label_smoothing, z_loss) if (label_smoothing != 0.0 or z_loss != 0.0) else (0.0, 0.0)

    def loss(self, input_ids, target_ids, criterion=None, start_pos: int = 0, ignore_index=None, segment_ids=None, *,
             label_smoothing=0.0, z_loss=0.0):
        """Cross entropy of the next-token logits.  `segment_ids` ((B, L) integers, non-decreasing along a row; a NumPy
        array, or an int32 device array a captured step re-reads at every replay): the documents of packed rows -- every
        attention looks inside the query's document only (core/fused/segments.py; llm/packing.py builds such rows and
        their targets).  Training mode and start_pos 0 only.  `criterion.ignore_index` (nn.CrossEntropyLoss), or the `ignore_index`
        keyword when no criterion is given: targets equal to it -- a prompt region, right padding -- add nothing to the loss
        or the gradients and the mean runs over the remaining tokens (core/fused/masked_loss.py; 0, not NaN, when none
        remains).  Under data parallel each rank divides by its own count.
        `label_smoothing` (in [0, 1]) and `z_loss` (>= 0; adds z_loss * logsumexp^2 per token, which keeps the lm_head's
        normaliser near 1), keywords or carried by the criterion likewise: core/fused/smooth_loss.py; with `ignore_index` both
        terms are averaged over the same remaining tokens.  Both 0: the step of before."""
        if criterion is not None and ignore_index is not None:
            raise ValueError("pass ignore_index through the criterion (nn.CrossEntropyLoss(ignore_index=...)), not beside it")
        eps, lam = self._smoothing(criterion, label_smoothing, z_loss)
        if criterion is not None:
            ignore_index = getattr(criterion, "ignore_index", None)
        h = self._forward_hidden(input_ids, start_pos) if segment_ids is None else \
            self._forward_hidden(input_ids, start_pos, segment_ids=segment_ids)
        if isinstance(target_ids, Tensor):
            targets = target_ids.reshape(-1)
        else:
            targets = Tensor(np.asarray(target_ids).reshape(-1), dtype=np.int64, device=h.device)
        head = self.lm_head
        bias = getattr(head, "bias", None)
        reduction = getattr(criterion, "reduction", "mean") if criterion is not None else "mean"
        if ((criterion is None or type(criterion) is nn.CrossEntropyLoss) and type(head) is nn.Linear
                and fused.linear_cross_entropy.applicable(h, head.weight, bias, targets, reduction, ignore_index)):
            # lm_head + cross entropy as one node: the (tokens, vocab) gradient of the logits is never written
            if eps != 0.0 or lam != 0.0:
                return fused.linear_cross_entropy(h, head.weight, bias, targets, reduction, ignore_index, eps, lam)
            if ignore_index is None:
                return fused.linear_cross_entropy(h, head.weight, bias, targets, reduction)
            return fused.linear_cross_entropy(h, head.weight, bias, targets, reduction, ignore_index)
        logits = head(h)
        B, L, V = logits.shape
        if criterion is None and (eps != 0.0 or lam != 0.0):
            criterion = nn.CrossEntropyLoss(ignore_index=ignore_index, label_smoothing=eps, z_loss=lam)
        if criterion is None:
            criterion = nn.CrossEntropyLoss() if ignore_index is None else nn.CrossEntropyLoss(ignore_index=ignore_index)
        return criterion(logits.reshape(B * L, V), targets)

    def token_losses(self, input_ids, target_ids, start_pos: int = 0, ignore_index=None, segment_ids=None, *,
                     label_smoothing=0.0, z_loss=0.0):
        """The cross entropy of every next-token prediction, a (B, L) tensor on the tape, 0 at tokens whose target equals
        `ignore_index`; nothing is counted or divided (core/fused/row_loss.py).  What follows plain SFT is built from it
        with plain operators -- `(token_losses * w).sum() / w.sum()` for per-token or per-document weights, a sum per row
        for sequence log-probabilities -- and still ends in the one lm_head + loss node, whose backward then takes a
        different upstream gradient per token.  `segment_ids`, `label_smoothing`, `z_loss`: as in `loss` (the smoothed rows
        are no log-probabilities: `sequence_logprobs` and `preference_step` do not take them)."""
        eps, lam = self._smoothing(None, label_smoothing, z_loss)
        h = self._forward_hidden(input_ids, start_pos) if segment_ids is None else \
            self._forward_hidden(input_ids, start_pos, segment_ids=segment_ids)
        B, L = h.shape[0], h.shape[1]
        if isinstance(target_ids, Tensor):
            targets = target_ids.reshape(-1)
        else:
            targets = Tensor(np.asarray(target_ids).reshape(-1), dtype=np.int64, device=h.device)
        head = self.lm_head
        bias = getattr(head, "bias", None)
        if type(head) is nn.Linear and fused.linear_cross_entropy.applicable(h, head.weight, bias, targets, "none", ignore_index):
            if eps != 0.0 or lam != 0.0:
                rows = fused.linear_cross_entropy(h, head.weight, bias, targets, "none", ignore_index, eps, lam)
            else:
                rows = fused.linear_cross_entropy(h, head.weight, bias, targets, "none", ignore_index)
        else:
            logits = head(h)
            crit = nn.CrossEntropyLoss("none", ignore_index, eps, lam) if (eps != 0.0 or lam != 0.0) else \
                nn.CrossEntropyLoss("none", ignore_index)
            rows = crit(logits.reshape(B * L, logits.shape[-1]), targets)
        return rows.reshape(B, L)

    def sequence_logprobs(self, input_ids, target_ids, start_pos: int = 0, ignore_index=None, segment_ids=None):
        """log p(targets | inputs) of every row, (B,) on the tape: minus the sum of the row's `token_losses`."""
        return self.token_losses(input_ids, target_ids, start_pos, ignore_index, segment_ids).sum(-1) * -1.0

    def preference_step(self, chosen_ids, chosen_targets, rejected_ids, rejected_targets, ref_chosen_logps, ref_rejected_logps,
                        optimizer, beta=0.1, ignore_index=-100):
        """One DPO step (llm/preference.py): zero_grad -> ONE forward over the chosen and the rejected batch stacked to
        (2B, L), so one lm_head + loss node -> mean -logsigmoid(beta * ((pc - pr) - (rc - rr))) from plain operators on
        the (B,) sequence log-probabilities -> backward -> optimizer step; returns the loss.  `ref_*_logps`: the reference
        model's sequence log-probabilities, (B,) arrays or tensors without gradient."""
        from . import preference
        self.train(True)
        optimizer.zero_grad()
        host = lambda v: v.numpy() if isinstance(v, Tensor) else np.asarray(v)      # noqa: E731
        ids = np.concatenate([host(chosen_ids), host(rejected_ids)], 0)
        targets = np.concatenate([host(chosen_targets), host(rejected_targets)], 0)
        B = ids.shape[0] // 2
        logps = self.sequence_logprobs(ids, targets, ignore_index=ignore_index)
        loss = preference.dpo_loss_tensor(logps[:B], logps[B:], ref_chosen_logps, ref_rejected_logps, beta)
        loss.backward()
        optimizer.step()
        return loss.item()

    def finetune_step(self, input_ids, target_ids, optimizer, criterion=None, start_pos: int = 0, ignore_index=None,
                      segment_ids=None, *, label_smoothing=0.0, z_loss=0.0):
        """zero_grad -> forward -> cross entropy -> backward -> optimizer step; returns the loss.  `ignore_index`,
        `segment_ids`, `label_smoothing`, `z_loss`: see `loss`."""
        self.train(True)
        optimizer.zero_grad()
        if label_smoothing != 0.0 or z_loss != 0.0:
            kw = {} if segment_ids is None else {"segment_ids": segment_ids}
            loss = self.loss(input_ids, target_ids, criterion, start_pos, ignore_index, label_smoothing=label_smoothing,
                             z_loss=z_loss, **kw)
        elif segment_ids is None:
            loss = self.loss(input_ids, target_ids, criterion, start_pos, ignore_index)
        else:
            loss = self.loss(input_ids, target_ids, criterion, start_pos, ignore_index, segment_ids=segment_ids)
        loss.backward()
        optimizer.step()
        return loss.item()

    def forward(self, input_ids, start_pos: int):
        return self.lm_head(self._forward_hidden(input_ids, start_pos)[:, [-1], :])

    fast_decode = True      # class switch: False keeps every decode step on the generic tape-node path

    def generate(self, input_ids, max_new_tokens: int, temperature=0.0, top_k=0, top_p=1.0, seed=0,
                 repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logprobs=None, logit_bias=None,
                 allowed_token_ids=None, token_fsm=None):
        """Yield the next ids, (B, 1) int64, for positions L .. max_new_tokens - 1.  temperature 0 (the default): the
        greedy pick of the reference (model.py:258-269); temperature > 0: drawn with top-k / top-p and the seeded
        counter-based generator of llm/sampling.py (token at position t of row b: Philox counter (t, b)).
        `repetition_penalty` / `presence_penalty` / `frequency_penalty` (defaults: off): the penalties of llm/penalties.py
        on each row's logits -- its prompt's tokens and the tokens it generated -- before the pick or the draw.
        `logprobs` = n (an int in [0, 20]; None: off): every step yields (ids, lp) instead, lp an llm/logprobs.Logprobs
        of the row the pick or the draw read -- token (B, 1), top_ids (B, n), top_logprobs (B, n).
        `logit_bias` ({token id: bias}; -inf bans the token) / `allowed_token_ids` (the only tokens a row may produce):
        the edits of llm/logit_edits.py, after the penalties and before the pick or the draw -- one value for every row,
        or a sequence with one value (or None) per row.
        `token_fsm` (an llm/token_fsm.TokenFSM for every row, or a sequence with one or None per row): constrained
        decoding -- a row may only produce tokens its machine allows in its current state, which starts at the machine's
        start state and advances on every token the row produces; after the penalties, before the edits.
        The arguments are checked here, before anything runs."""
        temperature, top_k, top_p, seed = check_sampling_args(temperature, top_k, top_p, seed)
        penalty = pen_np.check_args(repetition_penalty, presence_penalty, frequency_penalty)
        n_lp = lp_np.check_n(logprobs)
        edit = edit_np.check_args(logit_bias, allowed_token_ids, 0, self.vocab_size, input_ids.shape[0])
        fsm = fsm_np.check_args(token_fsm, self.vocab_size, input_ids.shape[0])
        return self._generate(input_ids, max_new_tokens, (temperature, top_k, top_p, seed) if temperature > 0 else None,
                              penalty, n_lp, edit, fsm)

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
                        logprobs=None, logit_bias=None, allowed_token_ids=None, min_new_tokens=0, min_p=0.0,
                        token_fsm=None, stop_sequences=None):
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
        `logit_bias` / `allowed_token_ids`: as in `generate` (llm/logit_edits.py), one value or one per prompt;
        `min_new_tokens` = m: no row yields a stop id before it has produced m tokens (needs `stop_ids`).  Not with
        speculate > 0.
        `min_p` (llm/sampling.py; 0 = off): after top-k and top-p, only tokens whose probability is at least min_p times
        the largest stay in the draw.  Each of `temperature`, `top_k`, `top_p`, `seed` and `min_p` is one value or a
        sequence with one value per row, mixed freely: row b is then drawn with its own values, key (seed_b, 0) and
        counter (t, b); a row with temperature 0 in a run that samples takes the first maximum of its logits, and a run
        whose temperatures are all 0 is the greedy run.  The penalties stay one set of values for every row.
        `token_fsm`: as in `generate` (llm/token_fsm.py), one machine or one (or None) per prompt; a stopped row's state
        stays.  Not with speculate > 0.
        `stop_sequences` (llm/stop_sequences.py): a sequence of token-id sequences for every row, or a sequence with one
        such (or None) per prompt.  A row stops like at a stop id once the tokens it generated end in one of its
        sequences -- the token that completes the match is yielded, the row yields -1 from then on; prompt tokens never
        take part.  With `min_new_tokens` = m a match counts from the step at which a stop id could first be yielded.  The
        other rows' tokens do not change.  Not with speculate > 0.
        Every argument is checked here (ValueError), before anything runs."""
        V = self.vocab_size
        if int(max_new_tokens) != max_new_tokens or max_new_tokens < 0:
            raise ValueError(f"max_new_tokens must be a non-negative integer, got {max_new_tokens}")
        max_new_tokens = int(max_new_tokens)
        rows = [np.asarray(p.numpy() if isinstance(p, Tensor) else p).reshape(-1) for p in prompts]
        cache = self.layers[0].attention.cache_k
        if not rows:
            raise ValueError("generate_ragged needs at least one prompt")
        sampling = active_sampling(check_request_args(temperature, top_k, top_p, seed, min_p, len(rows), "row"))
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
        stopseq = ss_np.check_args(stop_sequences, V, len(rows), min_new_tokens, k)
        edit = edit_np.check_args(logit_bias, allowed_token_ids, min_new_tokens, V, len(rows), stops, k,
                                  stop_sequences=stopseq is not None)
        fsm = fsm_np.check_args(token_fsm, V, len(rows), k)
        self.last_speculation = None if k == 0 else spec_np.counts()
        if k:
            return self._speculate([r.astype(np.int64) for r in rows], max_new_tokens, k, sampling, stops)
        return self._generate_ragged([r.astype(np.int64) for r in rows], max_new_tokens, sampling, stops, penalty,
                                     n_lp, edit, fsm, stopseq)

    # -- decode fast path -----------------------------------------------------------
    graph_decode = True     # class switch: False issues the step's launches one by one instead of replaying a hipGraph
    decode_ahead = True     # class switch: False never queues the next step before the caller asked for it
    last_speculation = None  # the counts of the last generate_ragged(speculate=k > 0) run (llm/speculative.py)
    fused_decode = 2        # class switch: launches per layer = 2 (q|k|v inside the attention kernel), 1 -> 3, 0 / False -> 5
    wide_decode = True      # class switch: 9 .. 256 rows on the wide step (csrc/decode_wide.hip); False -> the generic step

    # -- continuous batching (serve): a finished row takes the next waiting request -------------------------------
    def serve(self, prompts, max_new_tokens, slots=None, temperature=0.0, top_k=0, top_p=1.0, seed=0, stop_ids=(),
              prefill_chunk=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logprobs=None,
              prefix_cache=False, logit_bias=None, allowed_token_ids=None, min_new_tokens=0, min_p=0.0,
              token_fsm=None, stop_sequences=None):
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
        hits, prompt_tokens, reused_tokens, copies, launches) as it goes; with the cache off it is left alone.
        `logit_bias` / `allowed_token_ids` (llm/logit_edits.py): one value for every request, or a sequence with one value
        (or None) per request -- a request's edits follow it into whichever row it runs in; `min_new_tokens` = m: no
        request yields a stop id before it has produced m tokens (needs `stop_ids`).
        `temperature` / `top_k` / `top_p` / `seed` / `min_p` (llm/sampling.py): each one value for every request, or a
        sequence with one value per request, mixed freely -- a greedy request (temperature 0) shares the batch with
        sampled ones, and two requests may differ in temperature or seed.  The promise above holds per request: request
        r's tokens are those of row r of `generate_ragged(prompts, max(budgets), <r's own values for every row>)`, drawn
        with key (seed_r, 0) and counter (t, r), whichever row it runs in and whatever the other requests' values are.
        The penalties are not per request: they stay one set of values for the call.
        `token_fsm` (llm/token_fsm.py): one machine for every request, or a sequence with one (or None) per request -- a
        request's machine follows it into whichever row it runs in, from its start state, with plain and chunked prefill
        and with the prefix cache.
        `stop_sequences` (llm/stop_sequences.py): a sequence of token-id sequences for every request, or a sequence with
        one such (or None) per request.  A request also ends, and frees its row for the next admission, once the tokens it
        generated end in one of its sequences (the matching tokens are yielded; prompt tokens never take part; with
        `min_new_tokens` = m a match counts from the step at which a stop id could first be yielded).  The match is made
        inside the replayed step, so a step queued ahead computes nothing for the row and writes nothing to its cache."""
        penalty = pen_np.check_args(repetition_penalty, presence_penalty, frequency_penalty)
        n_lp = lp_np.check_n(logprobs)
        k_pre = prefix_np.check_arg(prefix_cache, prefill_chunk)
        V = self.vocab_size
        rows = [np.asarray(p.numpy() if isinstance(p, Tensor) else p).reshape(-1) for p in prompts]
        if not rows:
            raise ValueError("serve needs at least one prompt")
        N = len(rows)
        sampling = active_sampling(check_request_args(temperature, top_k, top_p, seed, min_p, N))
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
        stopseq = ss_np.check_args(stop_sequences, V, N, min_new_tokens)
        edit = edit_np.check_args(logit_bias, allowed_token_ids, min_new_tokens, V, N, stops,
                                  stop_sequences=stopseq is not None)
        fsm = fsm_np.check_args(token_fsm, V, N)
        C = chunked.check_chunk(prefill_chunk, slots)
        if C is not None:
            return self._serve_chunked([p.astype(np.int64) for p in rows], budgets, int(slots), C, sampling, stops,
                                       penalty, n_lp, k_pre, edit, fsm, stopseq)
        return self._serve([p.astype(np.int64) for p in rows], budgets, int(slots), sampling, stops, penalty, n_lp, edit,
                           fsm, stopseq)

    def serve_all(self, prompts, max_new_tokens, slots=None, temperature=0.0, top_k=0, top_p=1.0, seed=0, stop_ids=(),
                  prefill_chunk=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                  logprobs=None, prefix_cache=False, logit_bias=None, allowed_token_ids=None, min_new_tokens=0,
                  min_p=0.0, token_fsm=None, stop_sequences=None):
        """`serve` run to the end: a list of N int64 arrays, request r's generated tokens in order -- cut after its first
        stop id or at the end of its first matching stop sequence, the matching tokens included.  `logprobs` = n: a
        list of (tokens, Logprobs) instead, the arrays of length k / (k, n) for a request's k tokens."""
        it = self.serve(prompts, max_new_tokens, slots, temperature, top_k, top_p, seed, stop_ids, prefill_chunk,
                        repetition_penalty, presence_penalty, frequency_penalty, logprobs, prefix_cache, logit_bias,
                        allowed_token_ids, min_new_tokens, min_p, token_fsm, stop_sequences)
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
        if self._fast_path(dev):
            out = self._beam_device(rows, n, W, length_penalty, stops)
        else:
            out = self._beam_module(rows, n, W, length_penalty, stops)
        # the rows' caches back to zeros, as a fresh model holds them: a later generation reads the slot after its prompt
        # before writing it (the reference's decode positions), so nothing of this search may stay there
        T = min(cache.shape[1], max(r.size for r in rows) + n + 1)
        for c in (c for layer in self.layers for c in (layer.attention.cache_k, layer.attention.cache_v)):
            c.data[:B, :T] = 0
        return out
