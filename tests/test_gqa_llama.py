"""`Llama(..., n_kv_heads=)`: a 2-layer grouped-query Llama (vocabulary 64, dim 128, 4 heads over 2 key/value heads of 32, ffn
256) at sequence 40, batch 2, on the emulated C ABI and (``-m gpu``) an MI355X, against the multi-head `Llama` whose K / V
weights are the grouped ones repeated per group: (a) loss and every parameter gradient of one backward (the multi-head K / V
weight gradients summed per group), (b) the KV-cache path -- a 7-token prompt and three one-token steps -- and a ragged
generation, both within the project's fp32 bound of 1e-4 relative; (c) the default n_kv_heads issues the step of a model
built without the argument, launch for launch."""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core import Tensor, fused
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam
from tests.abi_emulator import _gqa
from tests.conftest import device_variants
from tests.test_llama_golden import host
from tests.test_packed_llama import _RUNTIME

V, DIM, HEADS, KV, FFN, L, B, HD = 64, 128, 4, 2, 256, 40, 2, 32
G = HEADS // KV
_rng = np.random.default_rng(7)
IDS, TGT = _rng.integers(0, V, (B, L)), _rng.integers(0, V, B * L)


def _pair(dev):
    """The grouped model and its multi-head twin on `dev`."""
    _gqa.extend()                                         # (under the emulator: the pdnk_ entries)
    Graph.clear()
    np.random.seed(11)
    gq = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, n_kv_heads=KV)
    mh = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32)
    gq.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)     # (the table starts unset)
    src = dict(gq.named_parameters())
    for name, p in mh.named_parameters():
        w = src[name].data
        if w.shape != p.shape:                            # K / V: head j's columns repeated for heads j * G .. j * G + G - 1
            w = np.repeat(w.reshape(DIM, KV, 1, HD), G, axis=2).reshape(DIM, DIM)
        p.data[...] = w
    return gq.to(dev), mh.to(dev)


def _close(got, ref, what):
    err, size = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert got.shape == ref.shape and size > 0 and err <= 1e-4 * size, (what, err, size)


def _attention_nodes(t):
    seen, stack, found = set(), [t], []
    while stack:
        n = stack.pop()
        if id(n) not in seen:
            seen.add(id(n))
            found += [n] if isinstance(n, fused.attention) else []
            stack += [p for p in n.last if isinstance(p, Tensor)]
    return found


def check_gqa_llama(dev):
    gq, mh = _pair(dev)
    # (a) training path
    losses = []
    for m in (gq, mh):
        for p in m.parameters():
            p.zero_grad()
        loss = m.loss(IDS, TGT)
        if m is gq:
            nodes = _attention_nodes(loss)
            assert len(nodes) == 2 and all(n.last[1].shape == (B, L, KV, HD) for n in nodes)
            assert all(n._kind == "gqa" for n in nodes)                   # the shared-K/V kernels of include/pdn_gqattn.h
        loss.backward()
        losses.append(float(host(loss)))
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1])
    ref = dict(mh.named_parameters())
    for name, p in gq.named_parameters():
        if p.requires_grad:
            r = host(ref[name].grad)
            if r.shape != p.shape:
                r = r.reshape(DIM, KV, G, HD).sum(2).reshape(DIM, KV * HD)
            _close(host(p.grad), r, name)
    # (b) eval mode with the KV cache, and a ragged generation on the tape-node path
    try:
        for m in (gq, mh):
            m.eval()
        assert gq.layers[0].attention.cache_k.shape == (B, L, KV, HD) and not gq._fast_path(gq.lm_head.weight.device)
        for ids, pos in [(IDS[:, :7], 0)] + [(IDS[:, 7 + i:8 + i], 7 + i) for i in range(3)]:
            _close(host(gq.forward(ids, pos)), host(mh.forward(ids, pos)), f"logits at {pos}")
        steps = list(gq.generate_ragged([list(IDS[0, :5]), list(IDS[1, :9])], 3))
        assert len(steps) == 3 and all(host(s).shape == (B, 1) for s in steps)
    finally:
        gq.train(True)
        mh.train(True)


def check_default_kv_heads_issue_the_parents_step(dev):
    def one(**kw):
        Graph.clear()
        np.random.seed(5)
        m, lib = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, **kw), _lib.lib()
        m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)
        m.to(dev)
        opt = Adam(m.parameters(), lr=1e-3)
        m.finetune_step(IDS, TGT, opt)                    # (first step: allocations, tables)
        buf = (ctypes.c_int64 * 56)()
        lib.call("pdn_kernel_counters", buf, 56, 1)
        mark = len(getattr(lib, "calls", ()))
        loss = m.finetune_step(IDS, TGT, opt)
        lib.call("pdn_kernel_counters", buf, 56, 1)
        return loss, list(buf), [n for n in list(getattr(lib, "calls", ()))[mark:] if not any(k in n for k in _RUNTIME)]
    base, got = one(), one(n_kv_heads=HEADS)
    assert got == base and sum(base[1]) > 0 and base[1][55] == 0 and not any(n.startswith("pdnk_") for n in base[2])


for _f in (check_gqa_llama, check_default_kv_heads_issue_the_parents_step):
    device_variants(globals(), _f)
