"""CLIP (llm/clip/model.py of the reference) on this package's fused nodes: the transformer blocks and the whole model.

Same class names, constructor signatures and registered parameter names as the reference
(`mha.QKV.weight`, `mha.O.bias`, `layer_norm1.scale`, `mlp.fc1.weight`, ...), so weights map by name.
What differs is the node count: the reference's block is ~45 generic tape nodes; here
  MultiHeadAttention  one biased GEMM for the packed QKV projection, ONE attention node reading q / k / v
                      as strided views of it (streaming kernels, hd = 64, with or without the additive
                      causal mask tensor), one biased output GEMM
  CLIPLayerNorm       one last-axis LayerNorm node (9 generic nodes in the reference)
  MLP                 GEMM, one `x * sigmoid(1.702 x)` node, GEMM
  ImageEncoder        ONE patch-embedding node (patch projection + class token + position embedding, fused.patch_embed)
                      instead of a transposed image copy and four generic nodes; post_norm on the class rows only
  TextEncoder         the end-of-text rows gathered BEFORE post_norm (LayerNorm is per row: the same values, 77x fewer
                      rows normalised); their positions found on the host when the token ids are host data
  CLIP                the contrastive head as ONE node (fused.clip_logits: two L2 normalisations and the product)
The one deliberate extension: the reference's ImageEncoder concatenates a (1, 1, D) class token to (N, P, D) patches and
so only takes N = 1; here the class token is broadcast over the batch, row n being the single-image result for image n.
Weights: `pydynet_amd.llm.clip_io.load_model` maps an OpenAI ViT-B/32 state dict (any key -> array mapping) by the
reference's keys.  The tokenizer and the image preprocessing stay out of scope.
"""
import numpy as np

from .. import nn
from ..core import Tensor, fused, function as fn
from ..core.fused import patch_project  # noqa: F401  (llm/clip/model.py:17-32, on the generic operators)


def build_attention_mask(context_length: int):
    """Additive causal mask tensor (llm/clip/model.py:8-13): -inf above the diagonal."""
    mask = Tensor(np.triu(np.full((context_length, context_length), -np.inf, dtype=np.float32), 1), dtype=np.float32)
    mask.causal_pattern = True          # (the attention node then takes its causal flag instead of a general L x L mask)
    return mask


class MultiHeadAttention(nn.Module):
    def __init__(self, n_dim: int, n_heads: int):
        super().__init__()
        self.n_dim, self.n_heads, self.head_dim = n_dim, n_heads, n_dim // n_heads
        self.QKV = nn.Linear(n_dim, n_dim * 3, dtype=np.float32)
        self.O = nn.Linear(n_dim, n_dim, dtype=np.float32)

    def forward(self, x, mask):
        B, L, _ = x.shape
        xq, xk, xv = fn.split(self.QKV(x), 3, -1)                  # views into the packed projection
        shape = (B, L, self.n_heads, self.head_dim)
        causal = bool(getattr(mask, "causal_pattern", False)) and mask.shape == (L, L)
        if causal:
            mask = None                 # exactly the -inf upper triangle: the fused kernels' own causal flag
        elif mask is not None and mask.device != x.device:
            mask = Tensor(mask.numpy(), dtype=np.float32, device=x.device)
        ctx = fused.attention(xq.reshape(*shape), xk.reshape(*shape), xv.reshape(*shape), causal=causal, mask=mask)
        return self.O(ctx.reshape(B, L, -1))


class CLIPLayerNorm(nn.LayerNorm):
    """A conventional last-axis LayerNorm on the parameters of nn.LayerNorm (scale, shift); the running
    statistics the base class registers are not used (llm/clip/model.py:66-80)."""

    def __init__(self, normalized_shape, eps=0.000001, momentum=0.1, device=None, dtype=None):
        super().__init__(normalized_shape, eps, momentum, device, dtype)

    def forward(self, x):
        if len(self.normalized_shape) == 1 and x.shape[-1] == self.normalized_shape[0] and (
                not x.device.is_hip or (x.dtype == np.float32 and x.shape[-1] % 4 == 0 and x.shape[-1] <= 2048)):
            return fused.layer_norm(x, self.scale, self.shift, self.eps)
        mean = x.mean(axis=-1, keepdims=True)
        var = fn.square(x - mean).mean(axis=-1, keepdims=True)
        return (x - mean) / fn.sqrt(var + self.eps) * self.scale + self.shift


class MLP(nn.Module):
    def __init__(self, d_in: int, d_proj: int):
        super().__init__()
        self.d_in, self.d_proj = d_in, d_proj
        self.fc1 = nn.Linear(d_in, d_proj, dtype=np.float32)
        self.fc2 = nn.Linear(d_proj, d_in, dtype=np.float32)

    def forward(self, x):
        return self.fc2(fused.gated_sigmoid(self.fc1(x), 1.702))


class Transformer(nn.Module):
    def __init__(self, n_dim: int, n_head: int, mlp_dim: int):
        super().__init__()
        self.mha = MultiHeadAttention(n_dim, n_head)
        self.mlp = MLP(n_dim, mlp_dim)
        self.layer_norm1 = CLIPLayerNorm((n_dim,), eps=1e-5, dtype=np.float32)
        self.layer_norm2 = CLIPLayerNorm((n_dim,), eps=1e-5, dtype=np.float32)

    def forward(self, x, mask):
        x = x + self.mha(self.layer_norm1(x), mask)
        return x + self.mlp(self.layer_norm2(x))


class ImageEncoder(nn.Module):
    def __init__(self, n_dim, n_head, mlp_dim, kernel_size, n_layer, final_dim):
        super().__init__()
        self.kernel = nn.Parameter(Tensor(np.random.randn(n_dim, 3, kernel_size, kernel_size), dtype=np.float32))
        self.pre_norm = CLIPLayerNorm((n_dim,), 1e-5, dtype=np.float32)
        self.transformers = nn.ModuleList([Transformer(n_dim, n_head, mlp_dim) for _ in range(n_layer)])
        self.post_norm = CLIPLayerNorm((n_dim,), 1e-5, dtype=np.float32)
        self.proj = nn.Linear(n_dim, final_dim, bias=False, dtype=np.float32)

    def forward(self, x, class_emb, position_emb):
        x = fused.patch_embed(x, self.kernel, class_emb, position_emb)        # (N, P + 1, D)
        x = self.pre_norm(x)
        for block in self.transformers:
            x = block(x, None)
        return self.proj(self.post_norm(x[:, 0]))


class TextEncoder(nn.Module):
    def __init__(self, n_dim, n_head, mlp_dim, n_layer, final_dim, vocab_size):
        super().__init__()
        self.token_embed = nn.Embedding(vocab_size, n_dim, dtype=np.float32)
        self.transformers = nn.ModuleList([Transformer(n_dim, n_head, mlp_dim) for _ in range(n_layer)])
        self.post_norm = CLIPLayerNorm((n_dim,), 1e-5, dtype=np.float32)
        self.proj = nn.Linear(n_dim, final_dim, bias=False, dtype=np.float32)
        self._masks = {}

    def forward(self, idx, position_emb):
        """idx (B, L): token ids as a NumPy array or a Tensor on any device; the end-of-text token is the largest id."""
        ids = idx.data if isinstance(idx, Tensor) else np.asarray(idx)
        x = self.token_embed(idx) + position_emb
        B, L, D = x.shape
        mask = self._masks.get(L)
        if mask is None:
            mask = self._masks[L] = build_attention_mask(L)
        for block in self.transformers:
            x = block(x, mask)
        if isinstance(ids, np.ndarray):                  # host ids: the rows are known without touching the device
            rows = np.arange(B) * L + np.argmax(ids, axis=-1)
        else:                                            # device ids: found and used on the device (the library's
            # argmax reduces floating-point arrays; token ids < 2^24 are exact in float32)
            rows = ids.astype(np.float32).argmax(-1) + Tensor(np.arange(B) * L, dtype=np.int64, device=x.device).data
        return self.proj(self.post_norm(x.reshape(B * L, D)[rows]))


class CLIP(nn.Module):
    def __init__(self, image_dim: int = 768, image_heads: int = 12, image_mlp_dim: int = 3072, image_patch: int = 32,
                 image_layers: int = 12, text_dim: int = 512, text_heads: int = 8, text_mlp_dim: int = 2048,
                 text_layers: int = 12, final_dim: int = 512, vocab_size: int = 49408, vision_tokens: int = 50,
                 text_tokens: int = 77):
        super().__init__()
        self.class_embed = nn.Parameter(Tensor(np.random.randn(1, 1, image_dim), dtype=np.float32))
        self.v_pos_emb = nn.Parameter(Tensor(np.random.randn(vision_tokens, image_dim), dtype=np.float32))
        self.t_pos_emb = nn.Parameter(Tensor(np.random.randn(text_tokens, text_dim), dtype=np.float32))
        self.image_encoder = ImageEncoder(image_dim, image_heads, image_mlp_dim, image_patch, image_layers, final_dim)
        self.text_encoder = TextEncoder(text_dim, text_heads, text_mlp_dim, text_layers, final_dim, vocab_size)
        self.scale = 1                  # a Python number, or (load_model) a one-element Tensor

    def forward(self, img, idx):
        img_feature = self.image_encoder(img, self.class_embed, self.v_pos_emb)
        txt_feature = self.text_encoder(idx, self.t_pos_emb)
        scale = self.scale
        if isinstance(scale, Tensor) and scale.device != img_feature.device:
            scale = self.scale = scale.to(img_feature.device)      # moved once, not uploaded every step
        return fused.clip_logits(img_feature, txt_feature, scale)

    def set_trainable_parameters(self, trainable_prefixes=("text_encoder",)):
        """requires_grad = (the name starts with one of the prefixes) for every registered parameter, running statistics
        included, as the reference does (llm/clip/model.py:207-217); returns (trainable, frozen) counts."""
        trainable_count, frozen_count = 0, 0
        for name, param in self._parameters.items():
            is_trainable = any(name.startswith(prefix) for prefix in trainable_prefixes)
            param.requires_grad = is_trainable
            if is_trainable:
                trainable_count += 1
            else:
                frozen_count += 1
        return trainable_count, frozen_count

    def finetune_step(self, image, text_tokens, target_ids, optimizer, criterion=None):
        """zero_grad -> forward -> cross entropy over the (images, texts) logits -> backward -> optimizer step; returns the
        loss (llm/clip/model.py:219-243)."""
        if criterion is None:
            criterion = nn.CrossEntropyLoss()
        self.train(True)
        optimizer.zero_grad()
        logits = self(image, text_tokens)
        B, K = logits.shape
        targets = Tensor(np.asarray(target_ids).reshape(-1), dtype=np.int64, device=logits.device)
        loss = criterion(logits.reshape(B, K), targets)
        loss.backward()
        optimizer.step()
        return loss.item()
