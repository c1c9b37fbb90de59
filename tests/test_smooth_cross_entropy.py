"""label_smoothing and z_loss on the unfused cross-entropy node (F.cross_entropy_loss / nn.CrossEntropyLoss ->
fused.cross_entropy; pdnz_cross_entropy_fwd_f32 and pdnz_cross_entropy_bwd_f32 of include/pdn_smoothloss.h) against the float64
contract pydynet_amd/core/fused/smooth_loss.py, on the `cpu` device, on the emulated C ABI and (``-m gpu``) on a real MI355X.
Criterion: tests/test_linear_ce.py's `close` (1e-7 + 1e-4 of the float64 reference's largest entry).

Shapes (rows, V) are tests/test_row_cross_entropy.py's, one per dispatch variant of the forward and the backward: (7, 10)
streamed rows, no float4 (rows are not 16-byte aligned); (64, 32) and (64, 96) streamed rows in float4, one wave / more
elements than a wave; (300, 4096) rows through registers, more rows than workgroups; (33, 4100) above 4096 but streamed;
(70000, 8) more rows than the 65535 workgroups of the grid.  Reductions none / sum / mean; masks none / half / row 0 / last
row / all; ignore_index None / -100 / 0; (eps, lam) in {(0.3, 0), (0, 0.05), (0.3, 0.05)}.  'none' takes the upstream vectors
of that file (signed standard normal; zero on a third of the rows and all zero at (0.3, 0.05)) with NaN at every ignored
row.  The gradient is linear in the upstream number of a row, so ONE float64 gradient per (mask, eps, lam) serves all
reductions.  With both arguments zero the node issues the entries it issued before: equal counters, slot 45 stays 0."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
import pydynet_amd.nn.functional as F
from pydynet_amd import _lib, nn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import smooth_loss
from pydynet_amd.core.tensor import Graph
from tests.conftest import device_variants
from tests.test_linear_ce import close, host

SHAPES = [(7, 10), (64, 32), (64, 96), (300, 4096), (33, 4100), (70000, 8)]
MASKS = ("none", "half", "row 0", "last row", "all")
SMOOTH = [(0.3, 0.0), (0.0, 0.05), (0.3, 0.05)]
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
    from tests.abi_emulator import _loss, _rowloss, _smoothloss
    _loss.extend()
    _rowloss.extend()
    _smoothloss.extend()                                  # (under the emulator: the pdnz_ entries of include/pdn_smoothloss.h)


def _run(dev, rows, V, ignore_index):
    _extend()
    x0, t0, masks, ups = _problem(rows, V, ignore_index)
    for name, ignored in masks.items():
        if ignore_index is None and name != "none":
            continue
        t_np = t0 if ignore_index is None else np.where(ignored, ignore_index, t0)
        count = int((~ignored).sum())
        for eps, lam in SMOOTH:
            ref_rows = smooth_loss.rows(x0, t_np, eps, lam, ignore_index)
            ref_d1 = smooth_loss.dlogits(x0, t_np, 1.0, eps, lam, ignore_index)      # per unit of upstream: the gradient is linear in it
            for reduction, uname in [("none", "normal"), ("sum", None), ("mean", None)] + (
                    [("none", "third zero"), ("none", "zero")] if (eps, lam) == SMOOTH[-1] else []):
                what = f"{dev} ({rows}, {V}) ignore_index {ignore_index} {name} eps {eps} lam {lam} {reduction} u {uname}"
                Graph.clear()
                x = pdn.Tensor(x0, dtype=np.float32, device=dev, requires_grad=True)
                t = pdn.Tensor(t_np, dtype=np.int64, device=dev)
                if reduction == "mean" or uname == "normal":
                    out = nn.CrossEntropyLoss(reduction, ignore_index, label_smoothing=eps, z_loss=lam)(x, t)
                else:
                    out = F.cross_entropy_loss(x, t, reduction, ignore_index=ignore_index, label_smoothing=eps, z_loss=lam)
                assert type(out) is fused.cross_entropy and out.reduction == reduction and out.smooth
                if reduction == "none":
                    assert out.shape == (rows,)
                    u0 = np.where(ignored, np.float32(np.nan), ups[uname])       # NaN wherever the row is ignored
                    got_d = host(out.backward_all(pdn.Tensor(u0, dtype=np.float32, device=dev).data)[0])
                    ref_v, ref_d = ref_rows, ref_d1 * np.where(ignored, 0.0, ups[uname].astype(np.float64))[:, None]
                else:
                    (out * UPSTREAM).backward()
                    got_d = host(x.grad)
                    f = 1.0 if reduction == "sum" else (1.0 / count if count else 0.0)
                    ref_v, ref_d = np.array(ref_rows.sum() * f), ref_d1 * (UPSTREAM * f)
                got_v = np.asarray(host(out), np.float64).reshape(ref_v.shape)
                print(f"{what}: max |value err| {float(np.abs(got_v - ref_v).max()):.3e} of {float(np.abs(ref_v).max()):.3e}, "
                      f"max |dx err| {float(np.abs(got_d - ref_d).max()):.3e} of {float(np.abs(ref_d).max()):.3e}")
                close(got_v, ref_v, what + ": value")
                close(got_d, ref_d, what + ": dlogits")
                assert not got_d[ignored].any(), what + ": ignored rows are exactly 0"
                if reduction == "none":
                    assert not got_v[ignored].any(), what
                if uname == "zero" or ignored.all():
                    assert not got_d.any() and np.isfinite(got_d).all() and np.isfinite(got_v).all(), what
                if ignored.all():
                    assert not got_v.any(), what + ": no row left: the loss is 0"


CASES = [(r, v, i) for r, v in SHAPES for i in (-100, 0, None)]
IDS = [f"{r}x{v}-{i}" for r, v, i in CASES]


@pytest.mark.parametrize("rows,V,ignore_index", CASES, ids=IDS)
def test_smooth_cross_entropy_cpu(rows, V, ignore_index):
    _run("cpu", rows, V, ignore_index)


@pytest.mark.parametrize("rows,V,ignore_index", CASES, ids=IDS)
def test_smooth_cross_entropy_emulated(emulated_hip, rows, V, ignore_index):
    _run("hip:0", rows, V, ignore_index)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,V,ignore_index", CASES, ids=IDS)
def test_smooth_cross_entropy_gpu(hip, rows, V, ignore_index):
    _run("hip:0", rows, V, ignore_index)


def _counters():
    buf = (ctypes.c_int64 * 46)()
    _lib.lib().call("pdn_kernel_counters", buf, 46, 1)
    return list(buf)


def check_both_zero_is_the_node_of_before(dev):
    """label_smoothing == 0 and z_loss == 0, given or left out: the same entries, the same counters, the same bits, and
    nothing counted in slot 45; with one of them set slot 45 counts the forward and the backward entry"""
    _extend()
    L = _lib.lib()
    x0, t0, masks, _ = _problem(300, 4096, -100)
    seen, call = [], L.call

    def spy(name, *a):
        if name != "pdn_kernel_counters":
            seen.append(name)
        return call(name, *a)
    runs = {}
    L.call = spy
    try:
        for key, kw in (("default", {}), ("zeros", {"label_smoothing": 0.0, "z_loss": 0.0}), ("smooth", {"z_loss": 0.05})):
            for reduction, ignore_index in (("mean", None), ("mean", -100), ("none", -100)):
                t_np = t0 if ignore_index is None else np.where(masks["half"], ignore_index, t0)
                Graph.clear()
                x = pdn.Tensor(x0, dtype=np.float32, device=dev, requires_grad=True)
                _counters()
                del seen[:]
                out = F.cross_entropy_loss(x, pdn.Tensor(t_np, dtype=np.int64, device=dev), reduction, ignore_index=ignore_index, **kw)
                out.sum().backward()
                value, grad = host(out).copy(), host(x.grad).copy()
                runs[key, reduction, ignore_index] = ([n for n in seen if "cross_entropy" in n], _counters(), value, grad)
    finally:
        del L.call
    for (key, reduction, ignore_index), (names, cnt, value, grad) in runs.items():
        base = runs["default", reduction, ignore_index]
        if key == "smooth":
            assert names == ["pdnz_cross_entropy_fwd_f32", "pdnz_cross_entropy_bwd_f32"] and cnt[45] == 2, (names, cnt)
        else:
            assert not any(n.startswith("pdnz_") for n in names) and cnt[45] == 0, (names, cnt)
            assert names == base[0] and cnt == base[1], (key, names, base[0])
            assert np.array_equal(value, base[2]) and np.array_equal(grad, base[3])


device_variants(globals(), check_both_zero_is_the_node_of_before)


def check_bad_target(dev):
    """a valid target outside [0, V) raises the error the other forms raise, with and without ignore_index; a negative one
    does not wrap"""
    from pydynet_amd import hipnp
    _extend()
    for ignore_index in (-100, None):
        for wrong in (50, -1):
            Graph.clear()
            x = pdn.Tensor(np.zeros((37, 50), np.float32), device=dev, requires_grad=True)
            bad = np.arange(37) % 50
            bad[5] = wrong
            with pytest.raises(IndexError):
                F.cross_entropy_loss(x, pdn.Tensor(bad, dtype=np.int64, device=dev), "mean", ignore_index=ignore_index, z_loss=0.1)
                if dev != "cpu":
                    hipnp.check_index_errors()


device_variants(globals(), check_bad_target)


def test_bad_target_cpu():
    check_bad_target("cpu")


def test_surface_of_label_smoothing_and_z_loss():
    x = pdn.Tensor(np.zeros((4, 5), np.float32), requires_grad=True)
    t = pdn.Tensor(np.zeros(4, np.int64))
    onehot = pdn.Tensor(np.eye(5, dtype=np.float32)[:4])
    for kw in ({"label_smoothing": 0.1}, {"z_loss": 0.1}):
        with pytest.raises(ValueError, match="class-index"):
            F.cross_entropy_loss(x, onehot, **kw)
        with pytest.raises(ValueError, match="class-index"):
            nn.CrossEntropyLoss(**kw)(x, onehot)
    for kw in ({"label_smoothing": -0.1}, {"label_smoothing": 1.1}, {"z_loss": -1.0}):
        with pytest.raises(ValueError):
            F.cross_entropy_loss(x, t, **kw)
        with pytest.raises(ValueError):
            nn.CrossEntropyLoss(**kw)
        with pytest.raises(ValueError):
            fused.cross_entropy(x, t, **kw)
    crit = nn.CrossEntropyLoss("sum", 7, 0.2, 0.01)
    assert (crit.reduction, crit.ignore_index, crit.label_smoothing, crit.z_loss) == ("sum", 7, 0.2, 0.01)
    assert nn.CrossEntropyLoss().label_smoothing == 0.0 and nn.CrossEntropyLoss().z_loss == 0.0
    assert F.cross_entropy_loss(x, onehot).ndim == 0      # one-hot targets without the arguments: the reference's chain, as before
    # float64 predictions: the plain-operator expression of the same formula
    rng = np.random.default_rng(0)
    z0, t0 = rng.standard_normal((6, 5)), np.array([0, 4, 2, 2, 1, 3])
    for ignore_index in (None, 2):
        for reduction in ("none", "sum", "mean"):
            Graph.clear()
            z = pdn.Tensor(z0, dtype=np.float64, requires_grad=True)
            out = F.cross_entropy_loss(z, pdn.Tensor(t0, dtype=np.int64), reduction, ignore_index=ignore_index,
                                       label_smoothing=0.3, z_loss=0.05)
            assert type(out) is not fused.cross_entropy and out.dtype == np.float64
            u0 = rng.standard_normal(6) if reduction == "none" else np.array(0.7)
            (out * pdn.Tensor(u0, dtype=np.float64)).sum().backward()
            ref_v, ref_d = smooth_loss.cross_entropy(z0, t0, 0.3, 0.05, ignore_index, reduction, u0)
            np.testing.assert_allclose(host(out), ref_v, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(host(z.grad), ref_d, rtol=1e-12, atol=1e-12)
