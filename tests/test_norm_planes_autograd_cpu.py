"""The block norms' outputs never written, at node level on the emulated device: `qkv_attention` / `ffn_swiglu` behind a deferred
`rms_norm` call the projections of include/pdn_normplanes.h, hand the norm node the rows' statistics only (`_adopt_stats`: it
stays pending) and send the stacked weight gradient through `pdnp_norm_dw_blocks_f32`.  The row thresholds are lowered inside
each test and restored after.  Losses and gradients equal the path that writes the normalised rows; a later reader of
`norm.data` gets the right array, and the norm's backward keeps the adopted statistics."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core import fused
from pydynet_amd.core.tensor import Graph

D, F = 288, 192
NEW = ("pdnp_gateup_swiglu_norm_fwd_f32", "pdnp_qkv_rope_norm_fwd_f32", "pdnp_norm_dw_blocks_f32")
OLD = ("pdn_gateup_swiglu_norm_fwd_f32", "pdn_qkv_rope_norm_fwd_f32")


def host(x):
    return x.numpy() if isinstance(x, pdn.Tensor) else (x if isinstance(x, np.ndarray) else x.get())


def close(a, b, what, rt=1e-6):
    a, b = np.asarray(host(a), np.float64), np.asarray(host(b), np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)
    assert err <= rt, f"{what}: {err:.3e} of the largest entry"


@pytest.fixture
def lowered(emulated_hip, monkeypatch):
    """The emulator with the pdng_ and pdnp_ entries, every row threshold at 32, and a count of the calls of either family."""
    from tests.abi_emulator import _normgrad, _normplanes
    _normgrad.extend()
    emu = _normplanes.extend()
    cls = type(emu)
    monkeypatch.setattr(cls, "MIN_ROWS", 32)
    monkeypatch.setattr(cls, "_rowtile_takes", staticmethod(lambda M, pieces: True))    # (a statement about speed)
    monkeypatch.setattr(cls, "pdn_gemm_outres_blocks_supported",
                        lambda self, M, kb, nb: int(kb > 0 and kb % 32 == 0 and nb >= 1), raising=True)
    seen = {n: 0 for n in NEW + OLD}
    for name in NEW + OLD:
        def spy(self, *a, _f=getattr(cls, name), _n=name):
            seen[_n] += 1
            return _f(self, *a)
        monkeypatch.setattr(cls, name, spy)
    monkeypatch.setattr(fused.rms_norm, "fuse_bwd_min_rows", 32)
    monkeypatch.setattr(fused.rms_norm, "fold_min_rows", 32)
    monkeypatch.setattr(fused.ffn_swiglu, "epilogue_min_rows", 32)
    monkeypatch.setattr(fused.qkv_attention, "rope_min_rows", 32)
    monkeypatch.setattr(fused.qkv_attention, "norm_planes_min_rows", 32)
    monkeypatch.setattr(fused.ffn_swiglu, "norm_planes_min_rows", 32)
    return seen


def _switch(monkeypatch, on):
    monkeypatch.setattr(fused.ffn_swiglu, "norm_planes", on)
    monkeypatch.setattr(fused.qkv_attention, "norm_planes", on)


def _llama_step(on, monkeypatch):
    from pydynet_amd.llm.llama import Llama
    _switch(monkeypatch, on)
    Graph.clear()
    np.random.seed(8)
    V, H, Lq, B = 64, 6, 32, 8                              # 256 tokens
    model = Llama(V, D, H, 768, Lq, B, 1, np.float32)
    rng = np.random.default_rng(9)
    model.tok_embedding.weight.data[...] = (0.5 * rng.standard_normal((V, D))).astype(np.float32)
    for n, p_ in model.named_parameters():
        if n.endswith("norm.weight"):
            p_.data[...] = rng.uniform(0.5, 1.5, p_.shape).astype(np.float32)
    model.to("hip:0")
    from pydynet_amd.optim import Adam
    Adam(model.parameters(), lr=0.0).flatten_grads()       # equally spaced gradients: the stacked weight-gradient products
    ids, tgt = rng.integers(0, V, (B, Lq)), rng.integers(0, V, (B, Lq))
    loss = model.loss(ids, tgt)
    loss.backward()
    grads = {n: host(p_.grad) for n, p_ in model.named_parameters() if p_.requires_grad and p_.grad is not None}
    return float(host(loss)), grads


def test_llama_step_with_and_without_the_written_rows(lowered, monkeypatch):
    l1, g1 = _llama_step(True, monkeypatch)
    assert [lowered[n] for n in NEW] == [1, 1, 2] and [lowered[n] for n in OLD] == [1, 1], lowered   # (the new entries call the old)
    l0, g0 = _llama_step(False, monkeypatch)
    assert [lowered[n] for n in NEW] == [1, 1, 2] and [lowered[n] for n in OLD] == [2, 2], lowered
    assert abs(l1 - l0) <= 1e-6 * abs(l0), (l1, l0)
    assert g1.keys() == g0.keys() and len(g1) >= 10
    for n in g0:
        close(g1[n], g0[n], f"grad {n}")


class _Case:
    def __init__(self, hp, T=64, seed=0):
        rng = np.random.default_rng(seed)
        t = lambda a, rg: pdn.Tensor(a.astype(np.float32), dtype=np.float32, device="hip:0", requires_grad=rg)
        self.x0 = t(rng.standard_normal((T, D)), True)
        self.wn = t(rng.uniform(0.5, 1.5, D), True)
        self.buf = hp.from_numpy((0.08 * rng.standard_normal((2, D, F))).astype(np.float32))      # gate | up, equally spaced
        self.wg, self.wu = t(np.zeros((D, F)), True), t(np.zeros((D, F)), True)
        self.wg.data, self.wu.data = self.buf[0], self.buf[1]
        self.gbuf = hp.zeros((2, D, F), np.float32)          # ... and their gradients: the stacked product
        self.wg.grad, self.wu.grad = self.gbuf[0], self.gbuf[1]
        self.wd = t(0.08 * rng.standard_normal((F, D)), True)
        self.w2 = t(0.08 * rng.standard_normal((D, D)), True)
        self.c = t(rng.standard_normal((T, D)), False)

    def leaves(self):
        return {"x0": self.x0, "wn": self.wn, "wg": self.wg, "wu": self.wu, "wd": self.wd, "w2": self.w2}


def _run(build, on, monkeypatch, hp, **kw):
    _switch(monkeypatch, on)
    Graph.clear()
    case = _Case(hp, **kw)
    loss, extra = build(case)
    loss.backward()
    grads = {n: np.array(host(t.grad)) for n, t in case.leaves().items() if t.requires_grad and t.grad is not None}
    return float(host(loss)), grads, extra


def _both(build, lowered, monkeypatch, hp, expect_new, **kw):
    before = dict(lowered)
    l1, on, ex1 = _run(build, True, monkeypatch, hp, **kw)
    assert [lowered[n] - before[n] for n in NEW] == expect_new, lowered
    l0, off, ex0 = _run(build, False, monkeypatch, hp, **kw)
    assert [lowered[n] - before[n] for n in NEW] == expect_new, lowered
    assert abs(l1 - l0) <= 1e-6 * abs(l0)
    assert on.keys() == off.keys() and on
    for n in off:
        close(on[n], off[n], f"grad {n}")
    return ex1, ex0


def test_ffn_behind_a_norm(lowered, monkeypatch, emulated_hip):
    def build(c):
        n = fused.rms_norm(c.x0 * 1.5, c.wn)
        return (fused.ffn_swiglu(n, c.wg, c.wu, c.wd) * c.c).sum(), None
    _both(build, lowered, monkeypatch, emulated_hip, [1, 0, 1])


def test_reading_the_norm_after_the_forward(lowered, monkeypatch, emulated_hip):
    """the node stayed pending: `.data` runs its own kernel, and the backward still works from the adopted statistics"""
    def build(c):
        n = fused.rms_norm(c.x0 * 1.5, c.wn)
        y = fused.ffn_swiglu(n, c.wg, c.wu, c.wd)
        adopted = (n._x, n._rms) if n._stats_adopted else None
        got = np.array(host(n.data))                         # a late reader
        if adopted is not None:
            assert n._x is adopted[0] and n._rms is adopted[1] and n._pending is None
        x = 1.5 * host(c.x0.data).astype(np.float64)
        want = x / np.sqrt((x * x).mean(-1, keepdims=True) + n.eps) * host(c.wn.data)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
        return (y * c.c).sum() + ((n @ c.w2) * c.c).sum(), got
    got_on, got_off = _both(build, lowered, monkeypatch, emulated_hip, [1, 0, 1])
    close(got_on, got_off, "norm.data")


def test_weights_that_are_not_leaves_write_the_rows_after_all(lowered, monkeypatch, emulated_hip):
    def build(c):
        n = fused.rms_norm(c.x0 * 1.5, c.wn)
        return (fused.ffn_swiglu(n, c.wg * 1.0, c.wu * 1.0, c.wd) * c.c).sum(), None
    _both(build, lowered, monkeypatch, emulated_hip, [1, 0, 0])
