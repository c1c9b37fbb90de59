"""`segment_ids` through `Llama.loss` / `Llama.finetune_step`: the 1-layer Llama of tests/test_masked_llama.py (dim 288, 6 heads,
vocabulary 96) at sequence 64.  Emulated C ABI and (``-m gpu``) a real MI355X.

(a) the packing property: ONE row that packs documents of 20, 33 and 7 tokens and 4 of padding gives the masked mean loss and
    every parameter gradient of the three documents run separately at their own lengths, their 'sum' losses and gradients added
    and divided by the number of valid tokens -- positions are not reset, a rotary score depends on distances only.  The same
    row WITHOUT segment_ids does not: the test sees the mask;
(b) three Adam steps on packed rows against the same model on `cpu`;
(c) segment_ids=None issues exactly the entry points and the launch counters of a step built without the keyword; with
    segments the step's attention is the segmented one (counter slot 43), the persistent kernels' counters at rest;
(d) segments outside training at start_pos 0 are a ValueError."""
import ctypes

import numpy as np
import pytest

from pydynet_amd import nn
from pydynet_amd.core import fused
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.llm.packing import pack_sequences
from pydynet_amd.optim import Adam
from tests.conftest import device_variants
from tests.test_llama_golden import close, close_after_adam, host

V, DIM, HEADS, FFN, L = 96, 288, 6, 256, 64
IGNORE = -100
LR = 1e-3
DOCS = (20, 33, 7)                                        # + 4 of padding


def _model(dev, batch=1):
    Graph.clear()
    np.random.seed(5)
    m = Llama(V, DIM, HEADS, FFN, L, batch, 1, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)
    m.to(dev)
    return m


def _extend():
    from tests.abi_emulator import _loss, _segattn
    _loss.extend()                                        # (under the emulator: the pdnl_ and pdns_ entries)
    _segattn.extend()


def _counters():
    from pydynet_amd import _lib
    buf = (ctypes.c_int64 * 44)()
    _lib.lib().call("pdn_kernel_counters", buf, 44, 1)
    return list(buf)


def _grads(m):
    return {n: host(p.grad) for n, p in m.named_parameters() if p.requires_grad}


def check_packed_row_equals_the_documents_run_separately(dev):
    _extend()
    rng = np.random.default_rng(31)
    docs = [rng.integers(1, V, n) for n in DOCS]
    ids, tgt, seg = pack_sequences(docs, L, pad_id=0, ignore_index=IGNORE)
    assert ids.shape == (1, L) and list(np.bincount(seg[0])) == [20, 33, 7, 4]
    count = int((tgt != IGNORE).sum())
    assert count == sum(DOCS) - len(DOCS)
    # (both sides with the scatter-add embedding gradient: see tests/test_masked_llama.py)
    saved = fused.embedding.accumulate
    fused.embedding.accumulate = True
    try:
        def packed(**kw):
            m = _model(dev)
            for p in m.parameters():
                p.zero_grad()
            _counters()
            loss = m.loss(ids, tgt.reshape(-1), ignore_index=IGNORE, **kw)
            loss.backward()
            return float(host(loss)), _grads(m), _counters()
        loss, grads, cnt = packed(segment_ids=seg)
        assert cnt[43] == 2 and cnt[9] == 1 and cnt[10] == 1 and cnt[7] == cnt[8] == 0, cnt
        loss_plain, grads_plain, cnt_plain = packed()
        assert cnt_plain[43] == 0
        m = _model(dev)
        for p in m.parameters():
            p.zero_grad()
        total = 0.0
        for d in docs:                                    # each at its own length; the gradients add up in the leaves
            one = m.loss(d[None, :-1], d[1:], nn.CrossEntropyLoss("sum"))
            one.backward()
            total += float(host(one))
        ref = {n: g.astype(np.float64) / count for n, g in _grads(m).items()}
    finally:
        fused.embedding.accumulate = saved
    print("loss", loss, "separately", total / count, "packed without segments", loss_plain)
    close(np.array(loss), np.array(total / count), what="loss")
    assert set(grads) == set(ref) and len(ref) > 5
    for n in ref:
        close(grads[n], ref[n], atol=1e-7, what="grad " + n)
    # the same row under plain causal attention reads across the documents: it must NOT agree
    assert abs(loss_plain - total / count) > 1e-3 * abs(total / count), (loss_plain, total / count)
    n = "layers.0.attention.Q.weight"
    assert np.abs(grads_plain[n] - ref[n]).max() > 1e-2 * np.abs(ref[n]).max()


def _packed_batch(seed, rows=2):
    rng = np.random.default_rng(seed)
    docs = [rng.integers(1, V, n) for n in rng.integers(5, 40, 12)]
    ids, tgt, seg = pack_sequences(docs, L, pad_id=0, ignore_index=IGNORE)
    assert ids.shape[0] >= rows
    return ids[:rows], tgt[:rows], seg[:rows]


def check_three_adam_steps_on_packed_rows(dev):
    _extend()
    ids, tgt, seg = _packed_batch(32)

    def run(device, ids_kind):
        m = _model(device, 2)
        opt = Adam(m.parameters(), lr=LR)
        s = seg
        if ids_kind == "device":
            from pydynet_amd import hipnp as hp
            s = hp.asarray(seg.astype(np.int32))
        losses = [m.finetune_step(ids, tgt.reshape(-1), opt, ignore_index=IGNORE, segment_ids=s) for _ in range(3)]
        return losses, {n: host(p) for n, p in m.named_parameters()}
    ref_losses, ref_params = run("cpu", "host")
    assert ref_losses[2] < ref_losses[0]
    for kind in ("host", "device"):
        losses, params = run(dev, kind)
        print(kind, "losses", losses, "cpu", ref_losses)
        close(np.array(losses), np.array(ref_losses), what="losses")
        for n in params:
            close_after_adam(params[n], ref_params[n], LR, 3, "final " + n)


_RUNTIME = ("malloc", "free", "memcpy", "memset", "event", "stream", "synchronize", "pool")


def check_default_path_issues_the_same_entry_points(dev):
    from pydynet_amd import _lib
    ids, tgt, seg = _packed_batch(33)
    emu = _lib.lib()
    plain = np.where(tgt == IGNORE, 0, tgt).reshape(-1)   # (the steps without ignore_index: every target a class)

    def one(**kw):
        m = _model(dev, 2)
        opt = Adam(m.parameters(), lr=LR)
        m.finetune_step(ids, plain, opt)                  # (first step: allocations, tables)
        _counters()
        mark = len(getattr(emu, "calls", ()))
        loss = m.finetune_step(ids, tgt.reshape(-1) if "ignore_index" in kw else plain, opt, **kw)
        calls = [n for n in list(getattr(emu, "calls", ()))[mark:] if not any(k in n for k in _RUNTIME)]
        return loss, _counters(), calls
    base = one()
    got = one(segment_ids=None)
    assert got[0] == base[0] and got[1] == base[1] and got[2] == base[2]
    assert sum(base[1]) > 0 and base[1][43] == 0 and not any(n.startswith("pdns_") for n in base[2])
    # ... and the packed step: the bounds once, the segmented attention in the place of the persistent one, all else the same
    _extend()
    packed = one(ignore_index=IGNORE, segment_ids=seg)
    masked = one(ignore_index=IGNORE)
    want = list(masked[1])
    assert want[7] + want[9] == 1 and want[8] + want[10] == 1 and want[43] == 0
    want[7], want[8], want[9], want[10], want[43] = 0, 0, 1, 1, 2
    assert packed[1] == want, (packed[1], want)
    if packed[2]:
        assert [n for n in packed[2] if n.startswith("pdns_")] == ["pdns_segment_bounds_i32", "pdns_attention_fwd_f32",
                                                                  "pdns_attention_bwd_f32"]
        assert [n for n in packed[2] if not n.startswith("pdns_")] == \
            [n for n in masked[2] if n not in ("pdn_attention_fwd_f32", "pdn_attention_bwd_rotated_f32", "pdn_attention_bwd_f32")]


def check_segments_are_for_training_rows(dev):
    _extend()
    ids, tgt, seg = _packed_batch(34)
    m = _model(dev, 2)
    with pytest.raises(ValueError, match="segment_ids"):
        m.loss(ids[:, 1:], tgt[:, 1:].reshape(-1), start_pos=1, ignore_index=IGNORE, segment_ids=seg[:, 1:])
    with pytest.raises(ValueError, match="segment_ids"):
        m.loss(ids, tgt.reshape(-1), ignore_index=IGNORE, segment_ids=seg[:, :-1])
    bad = seg.copy()
    bad[0, 30] = bad[0, 29] - 1
    with pytest.raises(ValueError, match="non-decreasing"):
        m.loss(ids, tgt.reshape(-1), ignore_index=IGNORE, segment_ids=bad)
    m.eval()                                              # (also switches gradient tracking off, process-wide)
    try:
        with pytest.raises(ValueError, match="segment_ids"):
            m.loss(ids, tgt.reshape(-1), ignore_index=IGNORE, segment_ids=seg)
    finally:
        m.train(True)


for _f in (check_packed_row_equals_the_documents_run_separately, check_three_adam_steps_on_packed_rows,
           check_default_path_issues_the_same_entry_points, check_segments_are_for_training_rows):
    device_variants(globals(), _f)
