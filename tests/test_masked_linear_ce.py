"""`ignore_index` on the lm_head + loss node (fused.linear_cross_entropy; C ABI pdnl_linear_ce_finish_f32 and
pdnl_linear_ce_backward_f32 of include/pdn_loss.h around the unchanged products) against the float64 contract
pydynet_amd/core/fused/masked_loss.py, under tests/test_linear_ce.py's criterion for the unmasked node on the same shapes
(1e-7 + 1e-4 of the reference's largest entry).  Emulated C ABI and (``-m gpu``) a real MI355X.

Shapes (rows, V) at D = 288, min_rows = 32: (64, 96) the smallest supported; (4096, 4000) the vocabulary cut into ranges by
both products; GPU only (32768, 4000), the fewest rows at which the split-fp16 forward, dx and dW forms all engage (asserted
through pdn_kernel_counters), and again with the three switched off for the fp32 forms.  Masks and ignore_index values are
tests/test_masked_cross_entropy.py's.  Every backward runs TWICE without zero_grad: the leaf gradients (dw_beta = db_beta = 1)
must hold twice the reference.  dx rows of ignored tokens are 0.0 exactly."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import nn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import chain, masked_loss
from pydynet_amd.core.tensor import Graph
from tests.test_linear_ce import close, host

D = 288
UPSTREAM = 0.5
MASKS = ("none", "half", "row 0", "last row", "all")


class _Problem:
    """inputs of one (rows, V, ignore_index) and the float64 logits, formed once and shared by its cases"""
    _cache = {}

    def __new__(cls, rows, V, ignore_index):
        key = (rows, V, ignore_index)
        if key not in cls._cache:
            cls._cache.clear()                            # (one at a time: the large one holds a GB of float64)
            p = cls._cache[key] = object.__new__(cls)
            rng = np.random.default_rng(rows + V)
            p.rows, p.V, p.ignore_index = rows, V, ignore_index
            p.x0 = rng.standard_normal((rows, D)).astype(np.float32)
            p.w0 = (0.05 * rng.standard_normal((D, V))).astype(np.float32)
            p.b0 = (0.1 * rng.standard_normal(V)).astype(np.float32)
            p.t0 = rng.integers(1 if ignore_index == 0 else 0, V, rows)
            p.t0[1:4] = (1, V - 1, V // 2)
            p.masks = {"none": np.zeros(rows, bool), "half": rng.random(rows) < 0.5, "row 0": np.arange(rows) == 0,
                       "last row": np.arange(rows) == rows - 1, "all": np.ones(rows, bool)}
            p.z = p.x0.astype(np.float64) @ p.w0.astype(np.float64) + p.b0
            p.refs = {}
        return cls._cache[key]

    def targets(self, mask):
        return np.where(self.masks[mask], self.ignore_index, self.t0)

    def reference(self, mask, reduction):
        """(loss, dx, dW, dbias) of ONE backward with upstream UPSTREAM, float64"""
        if (mask, reduction) not in self.refs:
            loss, d = masked_loss.cross_entropy(self.z, self.targets(mask), self.ignore_index, reduction, UPSTREAM)
            self.refs[mask, reduction] = (loss, d @ self.w0.astype(np.float64).T, self.x0.astype(np.float64).T @ d, d.sum(0))
        return self.refs[mask, reduction]


def _twice(dev, p, t_np, reduction, ignore_index, plain_operators=False):
    """loss and the gradients after TWO forward + backward passes without zero_grad in between"""
    Graph.clear()
    fused.linear_cross_entropy.min_rows = 32              # (as tests/test_linear_ce.py: the model takes the node from 32768 tokens up)
    head = nn.Linear(D, p.V, dtype=np.float32)
    head.weight.data[...] = p.w0
    head.bias.data[...] = p.b0
    head.to(dev)
    head.weight.zero_grad(); head.bias.zero_grad()
    x = pdn.Tensor(p.x0, dtype=np.float32, device=dev, requires_grad=True)
    t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
    for _ in range(2):
        h = x * 1.0                                       # a non-leaf input, as the final norm of the model is
        if plain_operators:
            built, relu_rows = chain.loss_chain.fused_built, fused.linear_relu.min_rows
            fused.linear_relu.min_rows = 1                # (as tests/test_loss_chain.py: the projection stays pending at any row count)
            try:
                loss = nn.CrossEntropyLoss(reduction, ignore_index)(head(h.reshape(2, p.rows // 2, D)).reshape(p.rows, p.V), t)
            finally:
                fused.linear_relu.min_rows = relu_rows
            assert chain.loss_chain.fused_built == built + 1
        elif ignore_index is None:
            loss = fused.linear_cross_entropy(h, head.weight, head.bias, t, reduction)
        else:
            assert fused.linear_cross_entropy.applicable(h, head.weight, head.bias, t, reduction, ignore_index)
            loss = fused.linear_cross_entropy(h, head.weight, head.bias, t, reduction, ignore_index)
        assert type(loss) is fused.linear_cross_entropy and loss.ignore_index == ignore_index
        (loss * UPSTREAM).backward()
    return float(host(loss)), host(x.grad), host(head.weight.grad), host(head.bias.grad)


def _check(got, ref, ignored, what):
    print(f"{what}: loss {got[0]:.7g} (float64 {ref[0]:.7g})", *(
        f"{n} err {float(np.abs(g - 2.0 * r).max()):.3e} of {float(np.abs(2.0 * r).max()):.3e}"
        for n, g, r in zip(("dx", "dW", "db"), got[1:], ref[1:])))
    close(np.array(got[0]), np.array(ref[0]), what + ": loss")
    for name, g, r in zip(("dx", "dW", "db"), got[1:], ref[1:]):
        close(g, 2.0 * r, f"{what}: {name} (two backward passes)")
    assert not got[1][ignored].any(), what + ": dx rows of ignored tokens are exactly 0"
    if ignored.all():
        assert got[0] == 0.0 and not got[2].any() and not got[3].any(), what


def _run(dev, rows, V, ignore_index, cases):
    from tests.abi_emulator import _loss
    _loss.extend()                                        # (under the emulator: the pdnl_ entries of include/pdn_loss.h)
    p = _Problem(rows, V, ignore_index)
    for mask, reduction in cases:
        got = _twice(dev, p, p.targets(mask), reduction, ignore_index)
        _check(got, p.reference(mask, reduction), p.masks[mask], f"{dev} ({rows}, {V}) ignore_index {ignore_index} {mask} {reduction}")
        if mask == "none":                                # nothing ignored: the unmasked node, within the same criterion
            plain = _twice(dev, p, p.t0, reduction, None)
            close(np.array(got[0]), np.array(plain[0]), "loss against the unmasked node")
            for name, g, u in zip(("dx", "dW", "db"), got[1:], plain[1:]):
                close(g, u, f"{name} against the unmasked node")
        if mask == "half":                                # nn.Linear -> reshape -> CrossEntropyLoss(ignore_index=...): the same node
            ops = _twice(dev, p, p.targets(mask), reduction, ignore_index, plain_operators=True)
            _check(ops, p.reference(mask, reduction), p.masks[mask], "plain operators")
            close(np.array(ops[0]), np.array(got[0]), "plain operators: loss against the node by name")
            for name, g, u in zip(("dx", "dW", "db"), ops[1:], got[1:]):
                close(g, u, f"plain operators: {name} against the node by name")


SMALL = [(m, r) for m in MASKS for r in ("mean", "sum")]
RANGES = [(m, "mean") for m in MASKS] + [("half", "sum")]


@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_masked_linear_ce_smallest_emulated(emulated_hip, ignore_index):
    _run("hip:0", 64, 96, ignore_index, SMALL)


@pytest.mark.parametrize("case", RANGES, ids=lambda c: "-".join(c).replace(" ", "_"))
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_masked_linear_ce_vocabulary_ranges_emulated(emulated_hip, ignore_index, case):
    _run("hip:0", 4096, 4000, ignore_index, [case])


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_masked_linear_ce_smallest_gpu(hip, ignore_index):
    _run("hip:0", 64, 96, ignore_index, SMALL)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RANGES, ids=lambda c: "-".join(c).replace(" ", "_"))
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_masked_linear_ce_vocabulary_ranges_gpu(hip, ignore_index, case):
    _run("hip:0", 4096, 4000, ignore_index, [case])


def _with(flags, fn):
    saved = {k: getattr(fused.linear_cross_entropy, k) for k in flags}
    for k, v in flags.items():
        setattr(fused.linear_cross_entropy, k, v)
    try:
        return fn()
    finally:
        for k, v in saved.items():
            setattr(fused.linear_cross_entropy, k, v)


FORMS = ({}, {"deferred_norm": False}, {"deferred_norm": False, "lse_epilogue": False})


def _forward_form(dev, flags):
    """the three ways the node finds its statistics (both products / the projection's store / a pass over the logits), each
    followed by the masked finish; the second and third form dx in the backward pass"""
    from tests.abi_emulator import _loss
    _loss.extend()
    p = _Problem(4096, 4000, -100)
    taken, fwd = [], fused.linear_cross_entropy.forward_

    def spy(node, *a):
        out = fwd(node, *a)
        taken.append((node.deferred, node.stats_in_gemm))
        return out
    fused.linear_cross_entropy.forward_ = spy
    try:
        got = _with(flags, lambda: _twice(dev, p, p.targets("half"), "mean", -100))
    finally:
        fused.linear_cross_entropy.forward_ = fwd
    print(flags, "(deferred, stats_in_gemm) =", taken)
    assert taken[0][0] is (not flags)                     # the default is the deferred form at this shape
    assert not (taken[0][1] and "lse_epilogue" in flags)
    _check(got, p.reference("half", "mean"), p.masks["half"], f"{dev} {flags}")


@pytest.mark.parametrize("flags", FORMS, ids=("deferred", "epilogue_or_pass", "pass"))
def test_masked_linear_ce_forward_form_emulated(emulated_hip, flags):
    _forward_form("hip:0", flags)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FORMS, ids=("deferred", "epilogue_or_pass", "pass"))
def test_masked_linear_ce_forward_form_gpu(hip, flags):
    _forward_form("hip:0", flags)


def _counters(reset):
    from pydynet_amd import _lib
    buf = (ctypes.c_int64 * 41)()
    _lib.lib().call("pdn_kernel_counters", buf, 41, 1 if reset else 0)
    return list(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False])
def test_masked_linear_ce_split_fp16_forms_gpu(hip, split):
    """32768 rows: the projection (slot 37), the input gradient (slot 39) and the weight gradient (slot 40) on split-fp16 MFMA
    around the masked finish and backward; with the three switches off the fp32 forms (slots 5, 12, 13 alone)."""
    rows, V = 32768, 4000
    p = _Problem(rows, V, -100)
    flags = {} if split else {"split_forward": False, "split_dx": False, "split_dw": False}
    _counters(True)
    got = _with(flags, lambda: _twice("hip:0", p, p.targets("half"), "mean", -100))
    cnt = _counters(True)
    print("counters 5, 12, 13, 37, 39, 40:", [cnt[i] for i in (5, 12, 13, 37, 39, 40)])
    assert cnt[5] == 2 and cnt[12] == 2 and cnt[13] == 2, cnt
    assert [cnt[37], cnt[39], cnt[40]] == ([2, 2, 2] if split else [0, 0, 0]), cnt
    _check(got, p.reference("half", "mean"), p.masks["half"], f"(32768, 4000) split {split}")
    if split:                                             # an in-range ignore_index: the sanitised targets keep the compare from matching
        p0 = _Problem(rows, V, 0)
        _check(_twice("hip:0", p0, p0.targets("half"), "sum", 0), p0.reference("half", "sum"), p0.masks["half"],
               "(32768, 4000) ignore_index 0 sum")
