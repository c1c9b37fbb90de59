"""Weight I/O of the CLIP model (reference: llm/clip/io.py:76-167).

`load_model(model, params)` reads any mapping from the OpenAI ViT-B/32 key names to arrays -- a dict, a local `np.load`
of an `.npz`, ... -- with the reference's keys and transposes: `in_proj_weight`, `out_proj.weight`, `c_fc.weight` and
`c_proj.weight` are stored (out, in) there and (in, out) here (nn/modules/linear.py:26-27); `logit_scale` becomes
`model.scale = exp(logit_scale)` as a one-element Tensor.  The layer count is the model's own (the reference hard-codes
12).  Nothing is downloaded.  `save_finetuned_parameters` / `load_finetuned_parameters` round-trip the trainable subset
under the registered parameter names (`text_encoder.proj.weight`, ...).  Works for parameters on any device.
"""
from __future__ import annotations

import numpy as np

from ..autograd import no_grad
from ..core import Tensor

# our name inside a Transformer block -> (OpenAI key suffix, stored transposed?)
_BLOCK_KEYS = (
    ("mha.QKV.weight", "attn.in_proj_weight", True),
    ("mha.QKV.bias", "attn.in_proj_bias", False),
    ("mha.O.weight", "attn.out_proj.weight", True),
    ("mha.O.bias", "attn.out_proj.bias", False),
    ("layer_norm1.scale", "ln_1.weight", False),
    ("layer_norm1.shift", "ln_1.bias", False),
    ("layer_norm2.scale", "ln_2.weight", False),
    ("layer_norm2.shift", "ln_2.bias", False),
    ("mlp.fc1.weight", "mlp.c_fc.weight", True),
    ("mlp.fc1.bias", "mlp.c_fc.bias", False),
    ("mlp.fc2.weight", "mlp.c_proj.weight", True),
    ("mlp.fc2.bias", "mlp.c_proj.bias", False),
)


def openai_key_map(image_layers: int, text_layers: int):
    """{our parameter name: (OpenAI key, transposed)} for a model with these layer counts."""
    table = {"class_embed": ("visual.class_embedding", False),
             "v_pos_emb": ("visual.positional_embedding", False),
             "t_pos_emb": ("positional_embedding", False),
             "image_encoder.kernel": ("visual.conv1.weight", False),
             "image_encoder.pre_norm.scale": ("visual.ln_pre.weight", False),
             "image_encoder.pre_norm.shift": ("visual.ln_pre.bias", False),
             "image_encoder.post_norm.scale": ("visual.ln_post.weight", False),
             "image_encoder.post_norm.shift": ("visual.ln_post.bias", False),
             "image_encoder.proj.weight": ("visual.proj", False),
             "text_encoder.token_embed.weight": ("token_embedding.weight", False),
             "text_encoder.post_norm.scale": ("ln_final.weight", False),
             "text_encoder.post_norm.shift": ("ln_final.bias", False),
             "text_encoder.proj.weight": ("text_projection", False)}
    for ours, theirs, layers in (("image_encoder", "visual.transformer.resblocks", image_layers),
                                 ("text_encoder", "transformer.resblocks", text_layers)):
        for i in range(layers):
            for name, key, tr in _BLOCK_KEYS:
                table[f"{ours}.transformers.{i}.{name}"] = (f"{theirs}.{i}.{key}", tr)
    return table


def _assign(param, value):
    value = np.asarray(value, dtype=np.float32)
    if value.size == param.size and value.shape != tuple(param.shape):
        value = value.reshape(param.shape)                  # (the (D,) class embedding into the (1, 1, D) parameter)
    if tuple(value.shape) != tuple(param.shape):
        raise ValueError(f"checkpoint tensor has shape {value.shape}, parameter expects {tuple(param.shape)}")
    param.data[...] = np.ascontiguousarray(value, dtype=param.dtype)


@no_grad()
def load_model(model, params):
    """Copy an OpenAI-keyed state dict into `model` (a `pydynet_amd.llm.clip.CLIP`); returns the model."""
    table = openai_key_map(len(model.image_encoder.transformers), len(model.text_encoder.transformers))
    missing = [key for key, _ in table.values() if key not in params]
    if "logit_scale" not in params:
        missing.append("logit_scale")
    if missing:
        raise KeyError(f"state dict lacks {len(missing)} CLIP keys, e.g. {missing[:3]}")
    for name, (key, tr) in table.items():
        value = np.asarray(params[key], dtype=np.float32)
        _assign(model._parameters[name], value.T if tr else value)
    scale = np.exp(np.asarray(params["logit_scale"], np.float32)).reshape(-1)[:1]
    model.scale = Tensor(scale, dtype=np.float32, device=model.class_embed.device)
    return model


@no_grad()
def save_finetuned_parameters(model, output_path: str):
    """Write every parameter with requires_grad to an `.npz` under its registered name (io.py:151-157)."""
    np.savez(output_path, **{name: p.numpy() for name, p in model._parameters.items() if p.requires_grad})


@no_grad()
def load_finetuned_parameters(model, finetuned_path: str):
    """Copy the parameters an `.npz` holds by name into `model` (io.py:160-167); returns the model."""
    weights = np.load(finetuned_path)
    for name, p in model._parameters.items():
        if name in weights:
            _assign(p, weights[name])
    return model
