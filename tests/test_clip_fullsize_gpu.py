"""The full-size ViT-B/32 CLIP (the reference's constructor defaults: 12 + 12 layers, 768 / 512 wide, 49408 tokens) on a
real MI355X against the same weights on the package's "cpu" device: logits, loss and every parameter gradient of one
finetune_step at one image and three texts, within 1e-4; and the image rows of a batch of four equal to four single-image
runs (the class token broadcast over the batch)."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.clip import CLIP
from pydynet_amd.optim import SGD
from tests.abi_emulator import counters

RT = 1e-4


def host(x):
    if isinstance(x, pdn.Tensor):
        return x.numpy()
    return x if isinstance(x, np.ndarray) else x.get()


def close(a, b, what, rt=RT):
    a, b = np.asarray(host(a), np.float64), np.asarray(host(b), np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = float(np.abs(a - b).max()), max(float(np.abs(b).max()), 1e-30)
    assert err <= 1e-7 + rt * scale, (what, err, scale)


def vit_b32(seed=0):
    np.random.seed(seed)
    m = CLIP()
    rng = np.random.default_rng(seed)
    for n, p in m._parameters.items():
        if p.requires_grad:
            w = 0.02 * rng.standard_normal(p.shape)
            p.data[...] = (w + 1.0 if n.endswith(".scale") else w).astype(np.float32)      # (LayerNorm scales near 1)
    return m


def inputs():
    rng = np.random.default_rng(1)
    img = rng.standard_normal((1, 3, 224, 224)).astype(np.float32)
    idx = rng.integers(1, 49000, (3, 77)).astype(np.int64)
    for r, e in enumerate((7, 76, 30)):
        idx[r, e] = 49407
        idx[r, e + 1:] = 0
    return img, idx, np.array([2], np.int64)


def step(m, dev, img, idx, tgt):
    Graph.clear()
    m.to(dev)
    opt = SGD(m.parameters(), lr=0.0)              # lr 0: the weights stay as they are, the gradients are kept
    with pdn.no_grad():
        logits = host(m(pdn.Tensor(img, device=dev), idx))
    loss = m.finetune_step(img, idx, tgt, opt)
    grads = {n: host(p.grad) for n, p in m._parameters.items() if p.requires_grad}
    return logits, loss, grads


@pytest.mark.gpu
def test_vit_b32_clip_step_hip_matches_cpu(hip):
    img, idx, tgt = inputs()
    logits_c, loss_c, grads_c = step(vit_b32(), "cpu", img, idx, tgt)
    counters()
    logits_h, loss_h, grads_h = step(vit_b32(), "hip:0", img, idx, tgt)
    c = counters()
    assert c[24] == 2 and c[25] == 1 and c[26] == 4 and c[27] == 2, c[24:]
    close(logits_h, logits_c, "logits")
    assert abs(loss_h - loss_c) <= RT * abs(loss_c), (loss_h, loss_c)
    assert len(grads_h) == len(grads_c) == 301
    for n in grads_c:
        close(grads_h[n], grads_c[n], f"grad {n}")


@pytest.mark.gpu
def test_vit_b32_image_batch_rows_equal_single_images(hip):
    Graph.clear()
    m = vit_b32(3).to("hip:0")
    imgs = np.random.default_rng(4).standard_normal((4, 3, 224, 224)).astype(np.float32)
    with pdn.no_grad():
        enc = m.image_encoder
        batch = host(enc(pdn.Tensor(imgs, device="hip:0"), m.class_embed, m.v_pos_emb))
        for n in range(4):
            one = host(enc(pdn.Tensor(imgs[n:n + 1], device="hip:0"), m.class_embed, m.v_pos_emb))
            close(batch[n:n + 1], one, f"image row {n}", rt=1e-5)
