"""`Llama(..., sliding_window=)`: a 2-layer Llama (vocabulary 64, dim 128, 4 heads of 32, ffn 256) at sequence 40, batch 2,
window 12, on `cpu`, the emulated C ABI and (``-m gpu``) an MI355X: (a) loss and every parameter gradient of one backward
against the same model on the `cpu` device, whose attention is the NumPy statement with the band mask (on `cpu` itself: that
statement against float64), (b) the KV-cache path -- a 20-token prompt and three one-token steps -- against one training-mode
forward over the 23 tokens, (c) a ragged generation, all within the project's fp32 bound of 1e-4 relative; (d) the default
sliding_window issues the step of a model built without the argument, launch for launch."""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core import Tensor, fused
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam
from tests.conftest import device_variants
from tests.test_band_attention_gpu import _ref
from tests.test_gqa_llama import _attention_nodes, _close
from tests.test_llama_golden import host
from tests.test_packed_llama import _RUNTIME

V, DIM, HEADS, FFN, L, B, W = 64, 128, 4, 256, 40, 2, 12
_rng = np.random.default_rng(7)
IDS, TGT = _rng.integers(0, V, (B, L)), _rng.integers(0, V, B * L)


def _model(dev, **kw):
    Graph.clear()
    np.random.seed(11)
    m = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, **kw)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)     # (the table starts unset)
    return m.to(dev)


def _loss_and_grads(m):
    for p in m.parameters():
        p.zero_grad()
    loss = m.loss(IDS, TGT)
    nodes = _attention_nodes(loss)
    loss.backward()
    return float(host(loss)), {n: host(p.grad) for n, p in m.named_parameters() if p.requires_grad}, nodes


def check_band_llama(dev):
    m = _model(dev, sliding_window=W)
    assert m.sliding_window == W and not m._fast_path(m.lm_head.weight.device)
    # (a) training path
    if dev == "cpu":
        q, k, v, w = (np.random.default_rng(3).standard_normal((4, 1, 30, 2, 16)).astype(np.float32))
        node = fused.attention(*(Tensor(a, requires_grad=True) for a in (q, k, v)), causal=True, window=7)
        (node * Tensor(w)).sum().backward()
        for what, a, b in zip("o dq dk dv".split(), [node.data] + [t.grad for t in node.last], _ref(q, k, v, w, 0, 7)):
            _close(a, b, what)
    else:
        loss, grads, nodes = _loss_and_grads(m)
        assert len(nodes) == 2 and all(n.window == W for n in nodes)
        if _lib.provides("pdnb_attention_fwd_f32"):       # (the device; the emulator runs the band as a mask)
            assert all(n._kind == "band" for n in nodes)
        ref_loss, ref_grads, _ = _loss_and_grads(_model("cpu", sliding_window=W))
        assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss)
        for name, g in grads.items():
            _close(g, ref_grads[name], name)
    # (b) the window through the KV cache and at Lq == 1, (c) a ragged generation on the tape-node path
    want = host(m.forward_logits(IDS[:, :23], 0))
    try:
        m.eval()
        for ids, pos in [(IDS[:, :20], 0)] + [(IDS[:, 20 + i:21 + i], 20 + i) for i in range(3)]:
            _close(host(m.forward(ids, pos))[:, 0], want[:, pos + ids.shape[1] - 1], f"logits at {pos}")
        steps = list(m.generate_ragged([list(IDS[0, :15]), list(IDS[1, :19])], 3))
        assert len(steps) == 3 and all(host(s).shape == (B, 1) for s in steps)
    finally:
        m.train(True)


def check_default_window_issues_the_parents_step(dev):
    def one(**kw):
        m, lib = _model(dev, **kw), _lib.lib()
        opt = Adam(m.parameters(), lr=1e-3)
        m.finetune_step(IDS, TGT, opt)                    # (first step: allocations, tables)
        buf = (ctypes.c_int64 * 58)()
        lib.call("pdn_kernel_counters", buf, 58, 1)
        mark = len(getattr(lib, "calls", ()))
        loss = m.finetune_step(IDS, TGT, opt)
        lib.call("pdn_kernel_counters", buf, 58, 1)
        return loss, list(buf), [n for n in list(getattr(lib, "calls", ()))[mark:] if not any(k in n for k in _RUNTIME)]
    base, got = one(), one(sliding_window=None)
    assert got == base and sum(base[1]) > 0 and base[1][57] == 0 and not any(n.startswith("pdnb_") for n in base[2])
    assert Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, sliding_window=L).sliding_window is None     # (hides no key)


def test_band_llama_cpu():
    check_band_llama("cpu")


for _f in (check_band_llama, check_default_window_issues_the_parents_step):
    device_variants(globals(), _f)
