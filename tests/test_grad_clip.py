"""Gradient clipping by global norm, AdamW and `nn.utils.clip_grad_norm_` through the front end: the fused HIP path
(csrc/optim.hip; the emulated ABI on CPU, the MI355X under -m gpu) against the array statement of optim/clip.py that the
`cpu` device runs.  Model: Linear(130, 130) -> ReLU -> Linear(130, 10), whose 16900-element weight crosses a chunk of the
optimizer's table (16384) and whose biases (130, 10) are tails far below one."""
import numpy as np
import pytest

import pydynet_amd as pdn
import pydynet_amd.nn as nn
import pydynet_amd.nn.functional as F
from pydynet_amd.core.tensor import Graph
from pydynet_amd.optim import SGD, Adam, AdamW

from tests.abi_emulator import _optim
from tests.conftest import device_variants

MAX_NORM = 0.05
RNG = np.random.default_rng(21)
# Inputs of 0.003: the comparison is between two implementations of forward and backward (the device's GEMMs, NumPy's), whose
# gradients differ by an absolute round-off d of about 3e-8 of their typical size.  Where an entry of the first layer's
# gradient cancels to below eps / sqrt(1 - beta2) = 3e-7, Adam's update is (lr a_t (1 - beta1) / eps) g = 3.2e5 g, so the
# parameters of the two runs part by 3.2e5 d: 1e-5 per step at the gradient size unit-scale inputs give (a handful of the
# 16900 entries, measured between two NumPy runs whose inputs differ by one ulp), 1e-6 and less at this one.
X = 0.003 * RNG.standard_normal((16, 130), dtype=np.float32)
Y = RNG.integers(0, 10, 16)


class MLP(nn.Module):
    def __init__(self):
        super().__init__()
        self.layer1 = nn.Linear(130, 130, dtype=np.float32)
        self.layer2 = nn.Linear(130, 10, dtype=np.float32)

    def forward(self, x):
        return self.layer2(F.relu(self.layer1(x)))


def host(a):
    return np.asarray(a) if isinstance(a, (np.ndarray, np.generic)) else a.get()


def build(dev, x=None):
    _optim.extend()                                   # (under the emulator: the pdnx_ entries of include/pdn_optim.h)
    Graph.clear()
    np.random.seed(5)
    net = MLP().to(dev)
    return net, pdn.Tensor(X if x is None else x, dtype=np.float32, device=dev), pdn.Tensor(Y, dtype=np.int64, device=dev)


def run(dev, make_opt, steps=4, extra64=False, x=None):
    """`steps` optimizer steps; returns (losses, parameters, gradient norm of every step, optimizer).  `extra64` adds a
    float64 parameter with a loss term of its own, so not every parameter qualifies for the fused path."""
    net, x, y = build(dev, x)
    params = list(net.parameters())
    if extra64:
        extra = pdn.Tensor(np.linspace(0.5, 1.5, 7), dtype=np.float64, device=dev, requires_grad=True)
        params.append(extra)
    opt = make_opt(params)
    losses, norms = [], []
    for _ in range(steps):
        opt.zero_grad()
        loss = F.cross_entropy_loss(net(x), y)
        loss.backward()
        if extra64:
            (extra * extra).sum().backward()
        opt.step()
        losses.append(loss.item())
        norms.append(None if opt.last_grad_norm is None else float(host(opt.last_grad_norm)))
    return losses, [p.numpy() for p in params], norms, opt


_cpu = {}


def on_cpu(name, make_opt, **kw):
    """The `cpu` device's run (the optim/clip.py path), computed once per configuration."""
    if name not in _cpu:
        _cpu[name] = run("cpu", make_opt, **kw)[:3]
    return _cpu[name]


def same_trajectory(got, ref):
    (l0, p0, _), (l1, p1, _) = got[:3], ref
    assert np.allclose(l0, l1, rtol=1e-5), (l0, l1)
    for a, b in zip(p0, p1):
        assert np.allclose(a, b, rtol=1e-4, atol=2e-6), float(np.abs(a - b).max())


def clipped_adam(params):
    return Adam(params, lr=1e-2, max_grad_norm=MAX_NORM)


def adamw(params):
    return AdamW(params, lr=1e-2, weight_decay=0.1)


def check_clipped_adam_equals_the_array_statement(dev):
    got = run(dev, clipped_adam)
    assert all(n > MAX_NORM for n in got[2]), got[2]                  # every step clipped
    ref = on_cpu("clipped", clipped_adam)
    assert np.allclose(got[2], ref[2], rtol=1e-5), (got[2], ref[2])
    same_trajectory(got, ref)
    assert got[3].skipped_steps() == 0 and got[3].t == 5


device_variants(globals(), check_clipped_adam_equals_the_array_statement)


def check_adamw_equals_the_array_statement_and_decouples_the_decay(dev):
    got = run(dev, adamw)
    same_trajectory(got, on_cpu("adamw", adamw))
    l2 = run(dev, lambda ps: Adam(ps, lr=1e-2, weight_decay=0.1))
    assert max(float(np.abs(a - b).max()) for a, b in zip(got[1], l2[1])) > 1e-4      # not the L2 form
    assert got[2] == [None] * 4                                        # no clipping: no norm is taken


device_variants(globals(), check_adamw_equals_the_array_statement_and_decouples_the_decay)


def check_unit_scale_inputs_agree_but_for_round_off_level_gradients(dev):
    """The same two comparisons at inputs of unit scale (see X above): where a gradient entry sits at round-off level the two
    implementations' Adam steps may differ by up to one step per iteration, so the bound is the one tests/test_graph_gpu.py
    and tests/test_distributed_cpu.py state for that case: at most one entry in 500 outside rtol 1e-4 / atol 2e-6, and none
    further apart than the steps taken times lr.  (Not every step clips here: the batch is fitted after two.)"""
    x1 = (X / np.float32(0.003)).astype(np.float32)
    for name, make in (("clipped1", clipped_adam), ("adamw1", adamw)):
        got, ref = run(dev, make, x=x1), on_cpu(name, make, x=x1)
        assert np.allclose(got[0], ref[0], rtol=1e-5), (got[0], ref[0])
        for a, b in zip(got[1], ref[1]):
            err = np.abs(a - b)
            bad = err > 2e-6 + 1e-4 * np.abs(b)
            print(name, a.shape, "outside", int(bad.sum()), "max", float(err.max()))
            assert bad.sum() <= max(1, a.size // 500) and err.max() <= 4 * 1e-2, (name, int(bad.sum()), float(err.max()))


device_variants(globals(), check_unit_scale_inputs_agree_but_for_round_off_level_gradients)


def check_clip_grad_norm_with_sgd(dev):
    from pydynet_amd.nn.utils import clip_grad_norm_
    net, x, y = build(dev)
    params = list(net.parameters())
    opt = SGD(params, lr=0.1)
    opt.zero_grad()
    F.cross_entropy_loss(net(x), y).backward()
    g0 = [host(p.grad).copy() for p in params]
    norm = float(np.sqrt(sum((g.astype(np.float64) ** 2).sum() for g in g0)))
    # max_norm = 0.9 * norm: the first call clips; a second call on the clipped gradients sees max_norm * norm / (norm + 1e-6)
    # and scales by 1 - (1e-6 / max_norm) * (1 - max_norm / norm) at the most, which stays under 1e-6 while norm >= 0.12
    assert norm >= 0.12, norm
    max_norm = 0.9 * norm
    with pytest.raises(ValueError):
        clip_grad_norm_(params, max_norm, norm_type=1)
    ret = clip_grad_norm_(params, max_norm)
    assert isinstance(ret, pdn.Tensor) and ret.shape == () and ret.device == params[0].device
    assert abs(ret.item() - norm) <= 2.5e-7 * norm
    coef = np.float32(max_norm / (norm + 1e-6))
    g1 = [host(p.grad).copy() for p in params]
    for a, b in zip(g1, g0):
        assert np.allclose(a, b * coef, rtol=1e-6, atol=0)
    again = clip_grad_norm_(params, max_norm)
    assert abs(again.item() - max_norm) <= 1e-5 * max_norm
    for a, b in zip(params, g1):
        assert np.allclose(host(a.grad), b, rtol=1e-6, atol=0)
    opt.step()                                                         # SGD then steps on the clipped gradients
    assert all(np.isfinite(p.numpy()).all() for p in params)


device_variants(globals(), check_clip_grad_norm_with_sgd)


def test_clip_grad_norm_with_sgd_cpu():
    check_clip_grad_norm_with_sgd("cpu")


def check_partly_fused_parameters_take_the_array_path_together(dev):
    """One float64 parameter: with clipping set, ALL parameters leave the fused path (one norm over the whole model)."""
    from pydynet_amd import _lib
    got = run(dev, clipped_adam, extra64=True)
    assert all(n > MAX_NORM for n in got[2]), got[2]
    same_trajectory(got, on_cpu("clipped64", clipped_adam, extra64=True))
    calls = getattr(_lib.lib(), "calls", None)
    if calls is not None:                                              # (the emulator's record of the entries called)
        assert not [c for c in calls if "adam" in c or "grad_norm" in c or "grad_scale" in c]


device_variants(globals(), check_partly_fused_parameters_take_the_array_path_together)


NEW_ENTRIES = ("pdnx_grad_norm_multi_f32", "pdnx_grad_scale_multi_f32", "pdnx_adam_multi_clip_f32", "pdnx_adam_multi_clip_tick_f32")


def test_default_adam_issues_the_entry_points_it_always_did(emulated_hip):
    from pydynet_amd import _lib
    run("hip:0", lambda ps: Adam(ps, lr=1e-2), steps=3)
    calls = _lib.lib().calls
    assert calls.count("pdn_adam_multi_f32") == 3
    assert not [c for c in calls if c in NEW_ENTRIES]


def test_clipped_adam_issues_norm_then_update(emulated_hip):
    from pydynet_amd import _lib
    run("hip:0", clipped_adam, steps=2)
    calls = [c for c in _lib.lib().calls if "adam" in c or c in NEW_ENTRIES]
    assert calls == ["pdnx_grad_norm_multi_f32", "pdnx_adam_multi_clip_f32"] * 2
    run("hip:0", adamw, steps=2)
    calls = [c for c in _lib.lib().calls if "adam" in c or c in NEW_ENTRIES]
    assert calls[4:] == ["pdnx_adam_multi_clip_f32"] * 2


def test_non_finite_gradient_skips_the_update_and_counts(emulated_hip):
    """A non-finite norm: p, m, v keep their bits, `skipped_steps()` counts, `t` still advances -- on the fused path and on
    the array path alike."""
    for dev in ("hip:0", "cpu"):
        net, x, y = build(dev)
        params = list(net.parameters())
        opt = clipped_adam(params)
        opt.zero_grad()
        F.cross_entropy_loss(net(x), y).backward()
        opt.step()
        before = [p.numpy() for p in params] + [host(a).copy() for a in opt.m + opt.v]
        for bad in (np.inf, np.nan):
            g = host(params[1].grad).copy()
            g[3] = bad
            params[1].grad[...] = g if dev == "cpu" else emulated_hip.from_numpy(g)
            opt.step()
        after = [p.numpy() for p in params] + [host(a).copy() for a in opt.m + opt.v]
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert opt.skipped_steps() == 2 and opt.t == 4


def test_bad_arguments():
    p = pdn.Tensor(np.ones(3, np.float32), dtype=np.float32, requires_grad=True)
    with pytest.raises(ValueError):
        Adam([p], max_grad_norm=0.0)
    assert AdamW([p]).weight_decay == 1e-2 and AdamW([p]).decoupled_weight_decay
    assert pdn.optim.AdamW is AdamW
