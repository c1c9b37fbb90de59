"""`Llama(..., dropout=, generator=)`: a 2-layer Llama (dim 96, 2 heads of 48, ffn 256, vocabulary 512) at sequence 64, batch 2,
on the emulated C ABI and (``-m gpu``) an MI355X: the dropout=0.1 step against `cpu` within 1e-4 relative (the project's fp32
parity bound; both start from Generator(0), so they draw the same masks), dropout=0.0 against a model built without the
argument, launch for launch, and eval mode and `score`, which run without dropout."""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam
from tests.abi_emulator import _dropout
from tests.conftest import device_variants
from tests.test_llama_golden import host
from tests.test_packed_llama import _RUNTIME

V, DIM, HEADS, FFN, L, B = 512, 96, 2, 256, 64, 2
NSLOT = 55


def _model(dev, **kw):
    _dropout.extend()                                     # (under the emulator: the pdnd_ entries)
    Graph.clear()
    np.random.seed(5)
    m = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, **kw)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)
    m.to(dev)
    return m


_rng = np.random.default_rng(41)
IDS, TGT = _rng.integers(0, V, (B, L)), _rng.integers(0, V, B * L)


def _counters():
    buf = (ctypes.c_int64 * NSLOT)()
    _lib.lib().call("pdn_kernel_counters", buf, NSLOT, 1)
    return list(buf)


def check_dropout_step_agrees_with_cpu(dev):
    ids, tgt = IDS, TGT

    def run(device):
        m = _model(device, dropout=0.1)
        for p in m.parameters():
            p.zero_grad()
        loss = m.loss(ids, tgt)
        loss.backward()
        grads = {n: host(p.grad) for n, p in m.named_parameters() if n in ("tok_embedding.weight", "layers.1.attention.O.weight")}
        return float(host(loss)), grads, m.generator.get_state()
    ref, got = run("cpu"), run(dev)
    assert ref[2] == got[2] == (0, 5 * (B * L * DIM // 4))    # the embedding and two residuals per layer
    assert abs(float(host(_model("cpu").loss(ids, tgt))) - ref[0]) > 1e-4 * abs(ref[0])      # (the masks are seen)
    assert abs(got[0] - ref[0]) <= 1e-4 * abs(ref[0]) and len(ref[1]) == 2
    for n, r in ref[1].items():
        err, size = float(np.abs(got[1][n] - r).max()), float(np.abs(r).max())
        assert size > 0 and err <= 1e-4 * size, (n, err, size)


def check_dropout_zero_issues_the_parents_step(dev):
    ids, tgt = IDS, TGT

    def one(**kw):
        m, emu = _model(dev, **kw), _lib.lib()
        opt = Adam(m.parameters(), lr=1e-3)
        m.finetune_step(ids, tgt, opt)                    # (first step: allocations, tables)
        _counters()
        mark = len(getattr(emu, "calls", ()))
        loss = m.finetune_step(ids, tgt, opt)
        calls = [n for n in list(getattr(emu, "calls", ()))[mark:] if not any(k in n for k in _RUNTIME)]
        return loss, _counters(), calls
    base, got = one(), one(dropout=0.0)
    assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2]
    assert sum(base[1]) > 0 and base[1][54] == 0 and not any(n.startswith("pdnd_") for n in base[2])
    on = one(dropout=0.1)                                 # claim, forward and backward of five dropout nodes: slot 54 on the
    launches = sum(n.startswith("pdnd_") for n in on[2]) if on[2] else on[1][54]         # device, the entries on the emulator
    assert launches == 3 * 5 and on[0] != base[0]


def check_eval_and_score_ignore_dropout(dev):
    ids = IDS
    logits, scores = [], []
    try:
        for kw in ({}, {"dropout": 0.1}):
            m = _model(dev, **kw)
            scores.append(m.score(ids).token)                 # (training mode borrowed for an inference pass)
            assert m.generator is None or m.generator.get_state() == (0, 0)
            m.eval()                                          # (also switches gradient tracking off, process-wide)
            logits.append(host(m.forward_logits(ids[:, :16])))
    finally:
        m.train(True)
    assert np.array_equal(logits[0], logits[1]) and np.isfinite(logits[0]).all()
    assert np.array_equal(scores[0], scores[1]) and np.isfinite(scores[0]).all()


for _f in (check_dropout_step_agrees_with_cpu, check_dropout_zero_issues_the_parents_step, check_eval_and_score_ignore_dropout):
    device_variants(globals(), _f)
