"""`Llama.token_losses`, `Llama.sequence_logprobs` and `Llama.preference_step`: a 1-layer Llama (vocabulary 96, dim 288, 6 heads,
ffn 768, sequence 32, batch 2) whose lm_head + loss is the fused node with reduction='none' (the row finish and backward of
include/pdn_rowloss.h).  Emulated C ABI and (``-m gpu``) a real MI355X; criterion tests/test_linear_ce.py's `close`.

(a) token_losses(...).mean() -> backward gives the loss and every parameter gradient of loss(); with ignore_index, sum() / count
    does the same;
(b) with segment_ids the values at the tokens of other documents are unchanged when one document's tokens change;
(c) a `Llama.loss` step with default arguments issues the entry points it issued before: slot 44 stays 0, and counters, entry
    names and loss equal those of a run in which every pdnr_ entry and every function of core/fused/row_loss.py raises;
(d) preference_step: value and gradients against this package's NumPy device running the same code and against the float64
    statement of llm/preference.py, on margins including +-30; after 5 steps at lr 1e-3 the mean margin pc - pr has grown;
(e) GPU only: the step (token_losses * w).sum() / w.sum() -> backward -> Adam captured in a hipnp.Graph with the weights and
    the targets in device buffers, both rewritten between replays, against the same steps issued eagerly."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib
from pydynet_amd.core import fused
from pydynet_amd.core.fused import row_loss
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import preference
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam
from tests.conftest import device_variants
from tests.test_linear_ce import close, host

V, DIM, HEADS, FFN, L, B = 96, 288, 6, 768, 32, 2
IGNORE = -100
LR = 1e-3


def _model(dev, batch=B):
    Graph.clear()
    np.random.seed(5)
    m = Llama(V, DIM, HEADS, FFN, L, batch, 1, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, DIM)).astype(np.float32)
    m.to(dev)
    m.train(True)
    return m


def _fused_nodes(fn):
    """fn() and the (reduction, ignore_index) of every linear_cross_entropy node it ran"""
    seen, fwd = [], fused.linear_cross_entropy.forward_

    def spy(node, *a):
        seen.append((node.reduction, node.ignore_index))
        return fwd(node, *a)
    saved = fused.linear_cross_entropy.min_rows
    fused.linear_cross_entropy.forward_, fused.linear_cross_entropy.min_rows = spy, 32
    try:
        return fn(), seen
    finally:
        fused.linear_cross_entropy.forward_, fused.linear_cross_entropy.min_rows = fwd, saved


def _extend():
    from tests.abi_emulator import _loss, _rowloss, _segattn
    _loss.extend()
    _segattn.extend()
    _rowloss.extend()                                     # (under the emulator: the pdnr_ entries of include/pdn_rowloss.h)


def _grads(m):
    return {n: host(p.grad) for n, p in m.named_parameters() if p.requires_grad}


def _backward(m, make_loss):
    for p in m.parameters():
        p.zero_grad()
    loss = make_loss(m)
    loss.backward()
    return float(host(loss)), _grads(m)


def check_token_losses_reduce_to_the_loss(dev):
    _extend()
    rng = np.random.default_rng(2)
    ids, tgt = rng.integers(0, V, (B, L)), rng.integers(0, V, (B, L))
    masked = tgt.copy()
    masked[0, :10], masked[1, :17] = IGNORE, IGNORE
    count = int((masked != IGNORE).sum())

    def run():
        out = {}
        out["loss"] = _backward(_model(dev), lambda m: m.loss(ids, tgt.reshape(-1)))
        out["rows mean"] = _backward(_model(dev), lambda m: m.token_losses(ids, tgt).mean())
        out["masked loss"] = _backward(_model(dev), lambda m: m.loss(ids, masked.reshape(-1), ignore_index=IGNORE))
        out["masked rows"] = _backward(_model(dev), lambda m: m.token_losses(ids, masked, ignore_index=IGNORE).sum() / float(count))
        m = _model(dev)
        rows = m.token_losses(ids, masked, ignore_index=IGNORE)
        logp = m.sequence_logprobs(ids, masked, ignore_index=IGNORE)
        assert rows.shape == (B, L) and logp.shape == (B,)
        out["values"] = (host(rows), host(logp))
        return out
    out, seen = _fused_nodes(run)
    assert seen == [("mean", None), ("none", None), ("mean", IGNORE), ("none", IGNORE), ("none", IGNORE), ("none", IGNORE)], seen
    for a, b in (("rows mean", "loss"), ("masked rows", "masked loss")):
        print(a, out[a][0], b, out[b][0])
        close(np.array(out[a][0]), np.array(out[b][0]), f"{a} against {b}")
        assert set(out[a][1]) == set(out[b][1]) and len(out[b][1]) > 5
        for n in out[b][1]:
            close(out[a][1][n], out[b][1][n], f"{a} against {b}: grad {n}")
    rows, logp = out["values"]
    assert not rows[masked == IGNORE].any() and (rows[masked != IGNORE] > 0).all()
    close(logp, -rows.astype(np.float64).sum(-1), "sequence_logprobs against -token_losses.sum(-1)")
    close(np.array(rows.astype(np.float64).sum() / count), np.array(out["masked loss"][0]), "values against the masked loss")


def check_segments_keep_other_documents_values(dev):
    _extend()
    rng = np.random.default_rng(3)
    ids, tgt = rng.integers(0, V, (B, L)), rng.integers(0, V, (B, L))
    seg = np.zeros((B, L), np.int64)
    seg[0, 12:], seg[0, 23:] = 1, 2                       # row 0: documents of 12, 11 and 9 tokens; row 1: one document
    other = ids.copy()
    other[0, 12:23] = (ids[0, 12:23] + 1 + rng.integers(0, V - 1, 11)) % V      # every token of document 1 changes

    def run():
        a = host(_model(dev).token_losses(ids, tgt, segment_ids=seg))
        b = host(_model(dev).token_losses(other, tgt, segment_ids=seg))
        c = host(_model(dev).token_losses(other, tgt))     # (without the documents the change reaches the tokens after it)
        return a, b, c
    (a, b, c), seen = _fused_nodes(run)
    assert seen == [("none", None)] * 3
    same = seg != 1
    same[1] = True
    assert np.array_equal(a[same], b[same]), float(np.abs(a - b)[same].max())
    assert (a[0, 12:23] != b[0, 12:23]).all()
    assert (c[0, 23:] != a[0, 23:]).any()


def _counters():
    buf = (ctypes.c_int64 * 45)()
    _lib.lib().call("pdn_kernel_counters", buf, 45, 1)
    return list(buf)


_RUNTIME = ("malloc", "free", "memcpy", "memset", "event", "stream", "synchronize", "pool")


def check_default_loss_step_issues_the_entry_points_of_before(dev):
    _extend()
    rng = np.random.default_rng(4)
    ids, tgt = rng.integers(0, V, (B, L)), rng.integers(0, V, B * L)
    emu = _lib.lib()

    def one():
        m = _model(dev)
        opt = Adam(m.parameters(), lr=LR)
        m.finetune_step(ids, tgt, opt)                    # (first step: allocations, tables)
        _counters()
        mark = len(getattr(emu, "calls", ()))
        loss = m.finetune_step(ids, tgt, opt)
        calls = [n for n in list(getattr(emu, "calls", ()))[mark:] if not any(k in n for k in _RUNTIME)]
        return loss, _counters(), calls
    base, seen = _fused_nodes(one)
    assert seen == [("mean", None)] * 2 and base[1][44] == 0 and base[1][12] == 1 and base[1][13] == 1
    assert not any(n.startswith("pdnr_") for n in base[2])

    def refuse(*a, **k):
        raise AssertionError("the row loss ran in a step that never asked for it")
    call, saved = emu.call, {n: getattr(row_loss, n) for n in ("valid_rows", "check_targets", "rows", "dlogits", "abs_max", "scale_rows")}
    emu.call = lambda name, *a: refuse() if name.startswith("pdnr_") else call(name, *a)
    for n in saved:
        setattr(row_loss, n, refuse)
    try:
        again, seen = _fused_nodes(one)
    finally:
        del emu.call
        for n, f in saved.items():
            setattr(row_loss, n, f)
    assert again[0] == base[0] and again[1] == base[1] and again[2] == base[2]
    # ... and a step on the rows runs the same products, the pdnr_ entries around them
    def rows_step():
        m = _model(dev)
        opt = Adam(m.parameters(), lr=LR)
        _counters()
        opt.zero_grad()
        m.token_losses(ids, tgt).mean().backward()
        opt.step()
        return _counters()
    cnt, seen = _fused_nodes(rows_step)
    assert seen == [("none", None)] and cnt[44] == 2 and cnt[12] == 1 and cnt[13] == 1, (seen, cnt[44], cnt[12], cnt[13])


def test_dpo_statement_and_tape():
    """llm/preference.py: the tape's loss and gradients against the float64 statement, margins 0, +-30 and +-80 at beta 1"""
    rng = np.random.default_rng(0)
    margins = np.array([0.0, 30.0, -30.0, 80.0, -80.0, 0.3, -2.0])
    pr, rc, rr = rng.standard_normal(7) - 40.0, rng.standard_normal(7) - 40.0, rng.standard_normal(7) - 40.0
    pc = pr + (rc - rr) + margins
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-5)):
        Graph.clear()
        tc = pdn.Tensor(pc, dtype=dtype, requires_grad=True)
        tr = pdn.Tensor(pr, dtype=dtype, requires_grad=True)
        loss = preference.dpo_loss_tensor(tc, tr, rc.astype(dtype), rr.astype(dtype), 1.0)
        loss.backward()
        ref = preference.dpo_loss(tc.numpy(), tr.numpy(), rc.astype(dtype), rr.astype(dtype), 1.0)
        assert np.isfinite(host(loss)) and np.isfinite(host(tc.grad)).all()
        np.testing.assert_allclose(float(host(loss)), ref[0], rtol=tol, atol=tol)
        np.testing.assert_allclose(host(tc.grad), ref[1], rtol=tol, atol=tol)
        np.testing.assert_allclose(host(tr.grad), ref[2], rtol=tol, atol=tol)
    exact = preference.dpo_loss([0.0], [0.0], [0.0], [0.0], 0.1)
    assert abs(exact[0] - np.log(2.0)) < 1e-15 and exact[1][0] == -0.05 and exact[2][0] == 0.05      # the derivative at margin 0 is 1/2
    big = preference.dpo_loss(pc, pr, rc, rr, 1.0)
    np.testing.assert_allclose(big[1][:5] * 7, [-0.5, -np.exp(-30.0), -1.0, -np.exp(-80.0), -1.0], rtol=1e-9)


def _pairs(seed):
    rng = np.random.default_rng(seed)
    cid, rid = rng.integers(0, V, (B, L)), rng.integers(0, V, (B, L))
    ct, rt = rng.integers(0, V, (B, L)), rng.integers(0, V, (B, L))
    ct[:, :9], rt[:, :9] = IGNORE, IGNORE                 # a shared prompt
    rt[1, 25:] = IGNORE                                   # a shorter rejected answer
    return cid, ct, rid, rt


def check_preference_step(dev):
    _extend()
    cid, ct, rid, rt = _pairs(6)
    ref_model = _model("cpu", 2 * B)
    pc0 = ref_model.sequence_logprobs(cid, ct, ignore_index=IGNORE).numpy().astype(np.float64)
    pr0 = ref_model.sequence_logprobs(rid, rt, ignore_index=IGNORE).numpy().astype(np.float64)

    def step(device, rc, rr, beta):
        m = _model(device, 2 * B)
        loss = m.preference_step(cid, ct, rid, rt, rc, rr, Adam(m.parameters(), lr=LR), beta=beta)
        return loss, _grads(m)
    for margins, beta in ((np.array([30.0, -30.0]), 1.0), (np.array([0.0, 4.0]), 0.1)):
        rc = pc0 - pr0 - margins                          # (rr = 0: the first step's margins are these)
        rr = np.zeros(B)
        (loss, grads), seen = _fused_nodes(lambda: step(dev, rc.astype(np.float32), rr.astype(np.float32), beta))
        assert seen == [("none", IGNORE)], seen           # ONE lm_head + loss node over the stacked (2B, L) batch
        cpu_loss, cpu_grads = step("cpu", rc.astype(np.float32), rr.astype(np.float32), beta)
        stated = preference.dpo_loss(pc0, pr0, rc.astype(np.float32), rr.astype(np.float32), beta)[0]
        print("margins", margins, "beta", beta, "loss", loss, "cpu", cpu_loss, "float64 statement", stated)
        close(np.array(loss), np.array(cpu_loss), "loss against the NumPy device")
        close(np.array(loss), np.array(stated), "loss against the float64 statement")
        assert set(grads) == set(cpu_grads) and len(grads) > 5
        for n in grads:
            close(grads[n], cpu_grads[n], f"margins {margins}: grad {n} against the NumPy device")

    def five():
        m = _model(dev, 2 * B)
        opt = Adam(m.parameters(), lr=LR)
        gap = lambda: float((host(m.sequence_logprobs(cid, ct, ignore_index=IGNORE)) -                     # noqa: E731
                             host(m.sequence_logprobs(rid, rt, ignore_index=IGNORE))).mean())
        before = gap()
        losses = [m.preference_step(cid, ct, rid, rt, pc0.astype(np.float32), pr0.astype(np.float32), opt) for _ in range(5)]
        return before, gap(), losses
    (before, after, losses), _ = _fused_nodes(five)
    print("mean pc - pr before", before, "after 5 steps", after, "losses", losses)
    assert after > before and losses[-1] < losses[0]
    assert abs(losses[0] - np.log(2.0)) < 1e-3           # the policy starts as its own reference: margin 0


for _f in (check_token_losses_reduce_to_the_loss, check_segments_keep_other_documents_values,
           check_default_loss_step_issues_the_entry_points_of_before, check_preference_step):
    device_variants(globals(), _f)


def _weighted_trajectory(hip, use_graph):
    """steps of (token_losses * w).sum() / w.sum() -> backward -> Adam over five (weights, targets) pairs"""
    rng = np.random.default_rng(8)
    ids = rng.integers(0, V, (B, L))
    tgts = rng.integers(0, V, (5, B, L))
    ws = rng.random((5, B, L)).astype(np.float32)
    tgts[1][rng.random((B, L)) < 0.5] = IGNORE
    ws[2] = 0.0
    ws[2, 1, 7] = 3.0                                     # a single weighted token
    tgts[3, 1] = IGNORE                                   # the whole second sequence
    ws[4] *= np.float32(2.0 ** -12)                       # small weights: the normalised copy of x in the weight gradient
    m = _model("hip:0")
    opt = Adam(m.parameters(), lr=LR)
    opt.flatten_grads()
    idd = pdn.Tensor(ids, dtype=np.int64, device="hip:0")
    tgd = pdn.Tensor(tgts[0], dtype=np.int64, device="hip:0")
    wd = pdn.Tensor(ws[0], dtype=np.float32, device="hip:0")

    def step():
        opt.zero_grad()
        loss = (m.token_losses(idd, tgd, ignore_index=IGNORE) * wd).sum() / wd.sum()
        loss.backward()
        opt.step()
        return loss

    def run():
        losses = []
        if use_graph:
            g = hip.Graph()
            loss = g.capture(step)                        # steps 1 and 2 on the first pair
            losses.append(loss.item())
            for t, w in zip(tgts[1:], ws[1:]):
                tgd.data[...] = hip.from_numpy(t)
                wd.data[...] = hip.from_numpy(w)
                g.replay()
                losses.append(loss.item())
            assert opt.t == 1 + 6
            g.destroy()
        else:
            step()
            losses.append(step().item())
            for t, w in zip(tgts[1:], ws[1:]):
                tgd.data[...] = hip.from_numpy(t)
                wd.data[...] = hip.from_numpy(w)
                losses.append(step().item())
        return losses
    losses, seen = _fused_nodes(run)
    assert seen and all(s == ("none", IGNORE) for s in seen), seen
    return losses, {n: p.numpy() for n, p in m.named_parameters()}


@pytest.mark.gpu
def test_replayed_weighted_steps_follow_the_weights_and_targets_buffers(hip):
    eager, replayed = _weighted_trajectory(hip, False), _weighted_trajectory(hip, True)
    print("eager", eager[0], "replayed", replayed[0])
    close(np.array(replayed[0]), np.array(eager[0]), "losses")
    assert len(set(np.round(eager[0], 3))) == 5           # five different pairs, five different losses
    for n in eager[1]:
        close(replayed[1][n], eager[1][n], "parameter " + n)
