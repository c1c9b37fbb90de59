"""reduction='none' on the unfused cross-entropy node (F.cross_entropy_loss / nn.CrossEntropyLoss -> fused.cross_entropy; the
forward entries that leave loss_row and lse_row, and pdnr_cross_entropy_bwd_rows_f32 of include/pdn_rowloss.h) against the
float64 contract pydynet_amd/core/fused/row_loss.py, on the `cpu` device, on the emulated C ABI and (``-m gpu``) on a real
MI355X.  Criterion: tests/test_linear_ce.py's `close` (1e-7 + 1e-4 of the float64 reference's largest entry).

Shapes (rows, V), one per dispatch variant of the forward and the backward: (7, 10) generic rows, no float4 (rows are not
16-byte aligned); (64, 32) at most 32 classes; (64, 96) generic rows in float4; (300, 4096) rows through registers, more rows
than workgroups; (33, 4100) above 4096 but streamed; (70000, 8) more rows than the 65535 workgroups of the grid.  (The
one-thread-per-row kernel for <= 32 classes, counter slot 18, belongs to the fused forward + backward entry, which 'none'
cannot take -- dlogits needs the upstream vector; 'none' goes through pdn[l]_cross_entropy_fwd_f32, whose every variant
writes the rows.)  Masks and ignore_index values (-100, and 0, an id inside the vocabulary) are
tests/test_masked_cross_entropy.py's; None (no masking) runs as well.  Upstream vectors: signed standard normal, zero on a
third of the rows, all zero.  rows.sum() reproduces the 'sum' node under every mask; rows.mean() reproduces the 'mean' node
where nothing is ignored (that node divides by the number of rows that remain, rows.mean() by all of them)."""
import numpy as np
import pytest

import pydynet_amd as pdn
import pydynet_amd.nn.functional as F
from pydynet_amd import nn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import masked_loss, row_loss
from pydynet_amd.core.tensor import Graph
from tests.test_linear_ce import close, host

SHAPES = [(7, 10), (64, 32), (64, 96), (300, 4096), (33, 4100), (70000, 8)]
MASKS = ("none", "half", "row 0", "last row", "all")
UPSTREAM = 0.5


def _problem(rows, V, ignore_index):
    rng = np.random.default_rng(rows + V)
    x0 = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
    t0 = rng.integers(1 if ignore_index == 0 else 0, V, rows)
    t0[1], t0[2] = 1, V - 1
    masks = {"none": np.zeros(rows, bool), "half": rng.random(rows) < 0.5, "row 0": np.arange(rows) == 0,
             "last row": np.arange(rows) == rows - 1, "all": np.ones(rows, bool)}
    u = rng.standard_normal(rows).astype(np.float32)
    ups = {"normal": u, "third zero": np.where(np.arange(rows) % 3 == 0, np.float32(0), u), "zero": np.zeros(rows, np.float32)}
    return x0, t0, masks, ups


def _extend():
    from tests.abi_emulator import _loss, _rowloss
    _loss.extend()
    _rowloss.extend()                                     # (under the emulator: the pdnr_ entries of include/pdn_rowloss.h)


def _run(dev, rows, V, ignore_index):
    _extend()
    x0, t0, masks, ups = _problem(rows, V, ignore_index)
    for name, ignored in masks.items():
        if ignore_index is None and name != "none":
            continue
        t_np = t0 if ignore_index is None else np.where(ignored, ignore_index, t0)
        ref_rows = row_loss.rows(x0, t_np, ignore_index)
        for uname, u0 in ups.items():
            what = f"{dev} ({rows}, {V}) ignore_index {ignore_index} {name} u {uname}"
            Graph.clear()
            x = pdn.Tensor(x0, dtype=np.float32, device=dev, requires_grad=True)
            t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
            u = pdn.Tensor(u0, dtype=np.float32, device=dev)
            if uname == "normal":
                per_row = nn.CrossEntropyLoss("none", ignore_index)(x, t)
            else:
                per_row = F.cross_entropy_loss(x, t, "none", ignore_index=ignore_index)
            assert type(per_row) is fused.cross_entropy and per_row.reduction == "none" and per_row.shape == (rows,)
            (per_row * u).sum().backward()
            ref_d = row_loss.dlogits(x0, t_np, u0, ignore_index)
            got_rows, got_d = host(per_row), host(x.grad)
            print(f"{what}: max |row err| {float(np.abs(got_rows - ref_rows).max()):.3e} of {float(np.abs(ref_rows).max()):.3e}, "
                  f"max |dx err| {float(np.abs(got_d - ref_d).max()):.3e} of {float(np.abs(ref_d).max()):.3e}")
            close(got_rows, ref_rows, what + ": rows")
            close(got_d, ref_d, what + ": dlogits")
            assert not got_rows[ignored].any() and not got_d[ignored].any(), what + ": ignored rows are exactly 0"
            if uname == "zero":
                assert not got_d.any() and np.isfinite(got_d).all(), what
        # the reductions from plain operators on the rows against the 'sum' and 'mean' nodes' float64 statement
        for reduction in ("sum", "mean") if not ignored.any() else ("sum",):
            Graph.clear()
            x = pdn.Tensor(x0, dtype=np.float32, device=dev, requires_grad=True)
            t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
            per_row = F.cross_entropy_loss(x, t, "none", ignore_index=ignore_index)
            loss = per_row.sum() if reduction == "sum" else per_row.mean()
            (loss * UPSTREAM).backward()
            ref_loss, ref_d = masked_loss.cross_entropy(x0, t_np, -100 if ignore_index is None else ignore_index, reduction,
                                                        UPSTREAM)
            close(np.array(float(host(loss))), np.array(ref_loss), f"{name}: rows.{reduction}() against the '{reduction}' node")
            close(x.grad, ref_d, f"{name}: gradient of rows.{reduction}() against the '{reduction}' node")


CASES = [(r, v, i) for r, v in SHAPES for i in (-100, 0, None)]
IDS = [f"{r}x{v}-{i}" for r, v, i in CASES]


@pytest.mark.parametrize("rows,V,ignore_index", CASES, ids=IDS)
def test_row_cross_entropy_cpu(rows, V, ignore_index):
    _run("cpu", rows, V, ignore_index)


@pytest.mark.parametrize("rows,V,ignore_index", CASES, ids=IDS)
def test_row_cross_entropy_emulated(emulated_hip, rows, V, ignore_index):
    _run("hip:0", rows, V, ignore_index)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,V,ignore_index", CASES, ids=IDS)
def test_row_cross_entropy_gpu(hip, rows, V, ignore_index):
    _run("hip:0", rows, V, ignore_index)


def _nan_upstream_and_bad_target(dev):
    """NaN in the upstream vector on ignored rows changes nothing (a select, not a product); a valid target outside [0, V)
    raises the error the other reductions raise, with and without ignore_index"""
    from pydynet_amd import hipnp
    _extend()
    x0, t0, masks, ups = _problem(64, 96, -100)
    ignored = masks["half"]
    t_np = np.where(ignored, -100, t0)
    u0 = np.where(ignored, np.float32(np.nan), ups["normal"])
    Graph.clear()
    x = pdn.Tensor(x0, dtype=np.float32, device=dev, requires_grad=True)
    per_row = F.cross_entropy_loss(x, pdn.Tensor(t_np, dtype=np.int64, device=dev), "none", ignore_index=-100)
    d = host(per_row.backward_all(pdn.Tensor(u0, dtype=np.float32, device=dev).data)[0])
    close(d, row_loss.dlogits(x0, t_np, u0, -100), "dlogits under NaN on ignored rows")
    assert not d[ignored].any()
    for ignore_index in (-100, None):
        Graph.clear()
        x = pdn.Tensor(np.zeros((37, 50), np.float32), device=dev, requires_grad=True)
        bad = np.arange(37) % 50
        bad[5] = 50
        with pytest.raises(IndexError):
            F.cross_entropy_loss(x, pdn.Tensor(bad, dtype=np.int64, device=dev), "none", ignore_index=ignore_index)
            if dev != "cpu":
                hipnp.check_index_errors()


def test_nan_upstream_and_bad_target_cpu():
    _nan_upstream_and_bad_target("cpu")


def test_nan_upstream_and_bad_target_emulated(emulated_hip):
    _nan_upstream_and_bad_target("hip:0")


@pytest.mark.gpu
def test_nan_upstream_and_bad_target_gpu(hip):
    _nan_upstream_and_bad_target("hip:0")


def test_surface_of_reduction_none():
    x = pdn.Tensor(np.zeros((4, 5), np.float32), requires_grad=True)
    onehot = pdn.Tensor(np.eye(5, dtype=np.float32)[:4])
    with pytest.raises(ValueError, match="none"):
        F.cross_entropy_loss(x, onehot, "none")
    with pytest.raises(ValueError, match="none"):
        nn.CrossEntropyLoss("none", ignore_index=0)(x, onehot)
    with pytest.raises(ValueError):
        F.cross_entropy_loss(x, pdn.Tensor(np.zeros(4, np.int64)), "batchmean")
    crit = nn.CrossEntropyLoss("none", 7)
    assert crit.reduction == "none" and crit.ignore_index == 7 and nn.CrossEntropyLoss().reduction == "mean"
    with pytest.raises(AssertionError):
        nn.MSELoss("none")                                # the other Loss subclasses are unchanged
    # float64 predictions: the plain-operator chain
    rng = np.random.default_rng(0)
    z0, t0 = rng.standard_normal((6, 5)), np.array([0, 4, 2, 2, 1, 3])
    for ignore_index in (None, 2):
        Graph.clear()
        z = pdn.Tensor(z0, dtype=np.float64, requires_grad=True)
        per_row = F.cross_entropy_loss(z, pdn.Tensor(t0, dtype=np.int64), "none", ignore_index=ignore_index)
        assert type(per_row) is not fused.cross_entropy and per_row.dtype == np.float64
        u0 = rng.standard_normal(6)
        (per_row * pdn.Tensor(u0, dtype=np.float64)).sum().backward()
        np.testing.assert_allclose(host(per_row), row_loss.rows(z0, t0, ignore_index), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(host(z.grad), row_loss.dlogits(z0, t0, u0, ignore_index), rtol=1e-12, atol=1e-12)
