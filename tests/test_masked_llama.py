"""`ignore_index` through `Llama.loss` / `Llama.finetune_step`: a 1-layer Llama (dim 288, 6 heads, vocabulary 96, sequence 32)
whose lm_head + loss is the fused node (fused.linear_cross_entropy with the masked finish and backward of include/pdn_loss.h).
Emulated C ABI and (``-m gpu``) a real MI355X.

(a) three Adam steps with the targets of a prompt region masked: losses and final parameters against the same model on `cpu`,
    under the criteria tests/test_llama_golden.py applies between devices;
(b) the padding property: a batch whose second sequence is right-padded from position 20 (targets there = ignore_index) gives
    the masked mean loss and every parameter gradient of the two sequences run separately at their own lengths, their 'sum'
    losses and gradients added and divided by the number of valid tokens -- causal attention never looks right;
(c) ignore_index=None issues exactly the entry points of a step built without the argument."""
import ctypes

import numpy as np

import pydynet_amd as pdn
from pydynet_amd import nn
from pydynet_amd.core import fused
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam
from tests.conftest import device_variants
from tests.test_llama_golden import close, close_after_adam, host

V, DIM, HEADS, FFN, L, B = 96, 288, 6, 256, 32, 2
IGNORE = -100
LR = 1e-3


def _model(dev):
    Graph.clear()
    np.random.seed(5)
    m = Llama(V, DIM, HEADS, FFN, L, B, 1, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)
    m.to(dev)
    return m


def _fused_nodes(fn):
    """fn() and the ignore_index of every linear_cross_entropy node it ran"""
    seen, fwd = [], fused.linear_cross_entropy.forward_

    def spy(node, *a):
        seen.append(node.ignore_index)
        return fwd(node, *a)
    saved = fused.linear_cross_entropy.min_rows
    fused.linear_cross_entropy.forward_, fused.linear_cross_entropy.min_rows = spy, 32
    try:
        return fn(), seen
    finally:
        fused.linear_cross_entropy.forward_, fused.linear_cross_entropy.min_rows = fwd, saved


def _extend():
    from tests.abi_emulator import _loss
    _loss.extend()                                        # (under the emulator: the pdnl_ entries of include/pdn_loss.h)


def check_masked_prompt_region_three_adam_steps(dev):
    _extend()
    rng = np.random.default_rng(2)
    ids = rng.integers(0, V, (B, L))
    tgt = rng.integers(0, V, (B, L))
    tgt[0, :10] = IGNORE                                  # the prompts: 10 and 17 tokens
    tgt[1, :17] = IGNORE

    def run(device, through_criterion):
        m = _model(device)
        opt = Adam(m.parameters(), lr=LR)
        if through_criterion:
            losses = [m.finetune_step(ids, tgt.reshape(-1), opt, nn.CrossEntropyLoss(ignore_index=IGNORE)) for _ in range(3)]
        else:
            losses = [m.finetune_step(ids, tgt.reshape(-1), opt, ignore_index=IGNORE) for _ in range(3)]
        return losses, {n: host(p) for n, p in m.named_parameters()}
    (losses, params), seen = _fused_nodes(lambda: run(dev, True))
    assert seen == [IGNORE] * 3, seen                     # the fused lm_head + loss node is still taken
    ref_losses, ref_params = run("cpu", False)
    print("losses", losses, "cpu", ref_losses)
    close(np.array(losses), np.array(ref_losses), what="losses")
    assert ref_losses[2] < ref_losses[0]
    for n in params:
        close_after_adam(params[n], ref_params[n], LR, 3, "final " + n)


def check_right_padding_equals_the_sequences_run_separately(dev):
    _extend()
    rng = np.random.default_rng(3)
    n2, pad = 20, 0
    ids = rng.integers(1, V, (B, L))
    tgt = rng.integers(0, V, (B, L))
    ids[1, n2:], tgt[1, n2:] = pad, IGNORE
    count = L + n2
    # the reference's embedding gradient ASSIGNS the last occurrence of an id (core/fused/dense.py: embedding); the property is
    # one of sums over tokens, so both sides run with the scatter-add form
    saved = fused.embedding.accumulate
    fused.embedding.accumulate = True
    try:
        def padded():
            m = _model(dev)
            for p in m.parameters():
                p.zero_grad()
            loss = m.loss(ids, tgt.reshape(-1), ignore_index=IGNORE)
            loss.backward()
            return float(host(loss)), {n: host(p.grad) for n, p in m.named_parameters() if p.requires_grad}
        (loss, grads), seen = _fused_nodes(padded)
        assert seen == [IGNORE], seen
        m = _model(dev)
        for p in m.parameters():
            p.zero_grad()
        total = 0.0
        for row, n in ((0, L), (1, n2)):                  # each at its own length; the gradients add up in the leaves
            one = m.loss(ids[row:row + 1, :n], tgt[row, :n], nn.CrossEntropyLoss("sum"))
            one.backward()
            total += float(host(one))
        ref = {n: host(p.grad).astype(np.float64) / count for n, p in m.named_parameters() if p.requires_grad}
    finally:
        fused.embedding.accumulate = saved
    print("loss", loss, "separately", total / count)
    close(np.array(loss), np.array(total / count), what="loss")
    assert set(grads) == set(ref) and len(ref) > 5
    for n in ref:
        close(grads[n], ref[n], atol=1e-7, what="grad " + n)


def _counters():
    from pydynet_amd import _lib
    buf = (ctypes.c_int64 * 43)()
    _lib.lib().call("pdn_kernel_counters", buf, 43, 1)
    return list(buf)


_RUNTIME = ("malloc", "free", "memcpy", "memset", "event", "stream", "synchronize", "pool")


def check_default_path_issues_the_same_entry_points(dev):
    from pydynet_amd import _lib
    rng = np.random.default_rng(4)
    ids, tgt = rng.integers(0, V, (B, L)), rng.integers(0, V, B * L)
    emu = _lib.lib()

    def one(**kw):
        m = _model(dev)
        opt = Adam(m.parameters(), lr=LR)
        m.finetune_step(ids, tgt, opt)                    # (first step: allocations, tables)
        _counters()
        mark = len(getattr(emu, "calls", ()))
        loss = m.finetune_step(ids, tgt, opt, **kw)
        # (the emulator's log of entry names, less the runtime's: allocations and read-backs depend on what the pools hold)
        calls = [n for n in list(getattr(emu, "calls", ()))[mark:] if not any(k in n for k in _RUNTIME)]
        return loss, _counters(), calls
    (base, seen) = _fused_nodes(lambda: one())
    assert seen == [None, None]
    for kw in ({"ignore_index": None}, {"criterion": nn.CrossEntropyLoss()}, {"criterion": nn.CrossEntropyLoss(ignore_index=None)}):
        got, seen = _fused_nodes(lambda: one(**kw))
        assert seen == [None, None]
        assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2], kw
    assert sum(base[1]) > 0 and not any(n.startswith("pdnl_") for n in base[2])
    assert base[1][12] == 1 and base[1][13] == 1          # the lm_head products of the unmasked node, once each
    # ... and the masked step runs the same products, its own entries around them
    _extend()
    masked, seen = _fused_nodes(lambda: one(ignore_index=IGNORE))
    assert seen == [None, IGNORE]
    assert masked[1] == base[1], (masked[1], base[1])
    if masked[2]:
        assert [n for n in masked[2] if n.startswith("pdnl_")] == ["pdnl_linear_ce_finish_f32", "pdnl_linear_ce_backward_f32"]


for _f in (check_masked_prompt_region_three_adam_steps, check_right_padding_equals_the_sequences_run_separately,
           check_default_path_issues_the_same_entry_points):
    device_variants(globals(), _f)
