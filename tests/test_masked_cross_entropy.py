"""`ignore_index` on the unfused cross-entropy node (F.cross_entropy_loss / nn.CrossEntropyLoss -> fused.cross_entropy; C ABI
pdnl_cross_entropy_* of include/pdn_loss.h) against the float64 contract pydynet_amd/core/fused/masked_loss.py, on the `cpu`
device (there also against torch wherever a row remains), on the emulated C ABI and (``-m gpu``) on a real MI355X.

Shapes (rows, V): (37, 50) the generic rows with V no multiple of 4; (300, 4096) the rows held in registers at their lower
edge, more rows than workgroups; (64, 33000) above the register limit.  Masks: nothing ignored, about half at random, only
row 0, only the last row, everything.  ignore_index: -100, and 0 with real targets that also hit columns 1 and V - 1.
Reductions: mean and sum, upstream gradient 0.5.  Tolerance: tests/test_linear_ce.py's for the unmasked node against float64
(1e-7 + 1e-4 of the largest entry) -- the arithmetic per valid row is the same; ignored gradient rows are 0.0 exactly."""
import numpy as np
import pytest

import pydynet_amd as pdn
import pydynet_amd.nn.functional as F
from pydynet_amd import nn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import masked_loss
from pydynet_amd.core.tensor import Graph
from tests.test_linear_ce import close, host

SHAPES = [(37, 50), (300, 4096), (64, 33000)]
UPSTREAM = 0.5


def _problem(rows, V, ignore_index):
    rng = np.random.default_rng(rows + V)
    x0 = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
    t0 = rng.integers(1 if ignore_index == 0 else 0, V, rows)
    t0[1], t0[2] = 1, V - 1
    masks = {"none": np.zeros(rows, bool), "half": rng.random(rows) < 0.5, "row 0": np.arange(rows) == 0,
             "last row": np.arange(rows) == rows - 1, "all": np.ones(rows, bool)}
    return x0, t0, masks


def _run(dev, rows, V, ignore_index, with_torch=False):
    from tests.abi_emulator import _loss
    _loss.extend()                                        # (under the emulator: the pdnl_ entries of include/pdn_loss.h)
    x0, t0, masks = _problem(rows, V, ignore_index)
    for name, ignored in masks.items():
        t_np = np.where(ignored, ignore_index, t0)
        for reduction in ("mean", "sum"):
            what = f"{name} {reduction}"
            Graph.clear()
            x = pdn.Tensor(x0, dtype=np.float32, device=dev, requires_grad=True)
            t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
            if reduction == "mean":
                loss = nn.CrossEntropyLoss(ignore_index=ignore_index)(x, t)
            else:
                loss = F.cross_entropy_loss(x, t, "sum", ignore_index=ignore_index)
            assert type(loss) is fused.cross_entropy and loss.ignore_index == ignore_index
            dx_dev = getattr(loss, "_dx", None)           # (HIP: written in the forward pass, its column sums in `_aux`)
            (loss * UPSTREAM).backward()
            ref_loss, ref_d = masked_loss.cross_entropy(x0, t_np, ignore_index, reduction, UPSTREAM)
            got_loss, got_d = float(host(loss)), host(x.grad)
            print(f"{dev} ({rows}, {V}) ignore_index {ignore_index} {what}: loss {got_loss:.7g} (float64 {ref_loss:.7g}), "
                  f"max |dx err| {float(np.abs(got_d - ref_d).max()):.3e} of {float(np.abs(ref_d).max()):.3e}")
            close(np.array(got_loss), np.array(ref_loss), what + ": loss")
            close(got_d, ref_d, what + ": dlogits")
            assert not got_d[ignored].any(), what + ": ignored gradient rows are exactly 0"
            if ignored.all():
                assert got_loss == 0.0 and not got_d.any(), what
            if dev != "cpu" and 4096 <= V <= 32768 and V % 4 == 0:
                aux = getattr(dx_dev, "_aux", None)
                assert aux is not None and aux[0] == "colsum", what + ": the column sums handed to the Linear"
                close(aux[1], ref_d.sum(0), what + ": colsum")
                close(aux[1], got_d.astype(np.float64).sum(0), what + ": colsum against the gradient itself")
            if with_torch and not ignored.all():
                import torch
                xt = torch.tensor(x0, requires_grad=True)
                lt = torch.nn.functional.cross_entropy(xt, torch.tensor(t_np), ignore_index=ignore_index, reduction=reduction)
                (lt * UPSTREAM).backward()
                close(np.array(got_loss), np.array(lt.item()), what + ": loss against torch")
                close(got_d, xt.grad.numpy(), what + ": dlogits against torch")


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_masked_cross_entropy_cpu(rows, V, ignore_index):
    _run("cpu", rows, V, ignore_index, with_torch=True)


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_masked_cross_entropy_emulated(emulated_hip, rows, V, ignore_index):
    _run("hip:0", rows, V, ignore_index)


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_masked_cross_entropy_gpu(hip, rows, V, ignore_index):
    _run("hip:0", rows, V, ignore_index)


def _forward_only_and_late_backward(dev):
    """the forward-only entry (no gradient asked for) and the backward entry on its own (a forward under no_grad's
    statistics reused): pdnl_cross_entropy_fwd_f32 / pdnl_cross_entropy_bwd_f32"""
    from tests.abi_emulator import _loss
    _loss.extend()
    for rows, V in SHAPES:
        x0, t0, masks = _problem(rows, V, -100)
        t_np = np.where(masks["half"], -100, t0)
        Graph.clear()
        x = pdn.Tensor(x0, dtype=np.float32, device=dev)
        t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
        loss = F.cross_entropy_loss(x, t, ignore_index=-100)
        ref_loss, ref_d = masked_loss.cross_entropy(x0, t_np, -100, "mean", UPSTREAM)
        close(np.array(float(host(loss))), np.array(ref_loss), "forward-only loss")
        if dev != "cpu":
            x.requires_grad = True
            loss.last = [x]
            g = pdn.Tensor(np.float32(UPSTREAM), dtype=np.float32, device=dev)
            d = loss.backward_all(g.data.reshape((1,)))[0]
            close(d, ref_d, "backward from the saved statistics")
            assert not host(d)[masks["half"]].any()


def test_forward_only_and_late_backward_cpu():
    _forward_only_and_late_backward("cpu")


def test_forward_only_and_late_backward_emulated(emulated_hip):
    _forward_only_and_late_backward("hip:0")


@pytest.mark.gpu
def test_forward_only_and_late_backward_gpu(hip):
    _forward_only_and_late_backward("hip:0")


def _bad_target(dev):
    """a target that is neither the index nor a class: the error the unmasked node raises (IndexError; on a HIP device from
    hipnp.check_index_errors()).  Negative targets do not wrap in the masked form."""
    from pydynet_amd import hipnp
    from tests.abi_emulator import _loss
    _loss.extend()
    for bad in (50, -1):
        Graph.clear()
        x = pdn.Tensor(np.zeros((37, 50), np.float32), device=dev, requires_grad=True)
        t_np = np.arange(37) % 50
        t_np[3], t_np[5] = -100, bad
        t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
        with pytest.raises(IndexError):
            F.cross_entropy_loss(x, t, ignore_index=-100)
            if dev != "cpu":
                hipnp.check_index_errors()
    if dev != "cpu":                                     # the unmasked node, the same way
        Graph.clear()
        x = pdn.Tensor(np.zeros((37, 50), np.float32), device=dev, requires_grad=True)
        t_np = np.arange(37) % 50
        t_np[5] = 50
        with pytest.raises(IndexError):
            F.cross_entropy_loss(x, pdn.Tensor(t_np, dtype=np.int64, device=dev))
            hipnp.check_index_errors()


def test_bad_target_cpu():
    _bad_target("cpu")


def test_bad_target_emulated(emulated_hip):
    _bad_target("hip:0")


@pytest.mark.gpu
def test_bad_target_gpu(hip):
    _bad_target("hip:0")


def test_soft_targets_with_ignore_index_raise():
    x = pdn.Tensor(np.zeros((4, 5), np.float32), requires_grad=True)
    onehot = pdn.Tensor(np.eye(5, dtype=np.float32)[:4])
    with pytest.raises(ValueError, match="ignore_index"):
        F.cross_entropy_loss(x, onehot, ignore_index=-100)
    with pytest.raises(ValueError, match="ignore_index"):
        nn.CrossEntropyLoss(ignore_index=0)(x, onehot)
    assert nn.CrossEntropyLoss().ignore_index is None and nn.CrossEntropyLoss("sum", 7).ignore_index == 7
    assert not hasattr(nn.MSELoss(), "ignore_index")      # the other Loss subclasses are unchanged
