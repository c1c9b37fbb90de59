"""The deferred input gradient (core/fused/_common.py: DeferredInputGrad) on the emulated device: `qkv_attention` /
`ffn_swiglu` hand an `rms_norm` input the product unformed, and that node's backward runs it through
`pdng_outres_blocks_nt_rmsnorm_bwd_f32`.  The row thresholds (`fuse_bwd_min_rows`, `fold_min_rows`, the epilogue thresholds) and
the emulated `pdn_gemm_outres_blocks_supported` (a statement about speed: 57089 rows and more) are lowered inside each test and
restored after.  A one-layer width-288 Llama step with the fusion on and off, then the cases in which the object has to be
materialised or must never be made: gradients equal the unfused path."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import _common
from pydynet_amd.core.tensor import Graph

D, F = 288, 192
ENTRY = "pdng_outres_blocks_nt_rmsnorm_bwd_f32"


def host(x):
    return x.numpy() if isinstance(x, pdn.Tensor) else (x if isinstance(x, np.ndarray) else x.get())


def close(a, b, what, rt=1e-6):
    a, b = np.asarray(host(a), np.float64), np.asarray(host(b), np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)
    assert err <= rt, f"{what}: {err:.3e} of the largest entry"


@pytest.fixture
def lowered(emulated_hip, monkeypatch):
    """The emulator with the pdng_ entries, every row threshold at 32, and counters of what ran."""
    from tests.abi_emulator import _normgrad
    emu = _normgrad.extend()
    cls = type(emu)
    monkeypatch.setattr(cls, "pdn_gemm_outres_blocks_supported",
                        lambda self, M, kb, nb: int(kb > 0 and kb % 32 == 0 and nb >= 1), raising=True)
    seen = {"fused": 0, "made": 0, "formed": 0}
    entry = cls.pdng_outres_blocks_nt_rmsnorm_bwd_f32

    def spy_entry(self, *a):
        seen["fused"] += 1
        return entry(self, *a)
    monkeypatch.setattr(cls, ENTRY, spy_entry)
    init, mat = _common.DeferredInputGrad.__init__, _common.DeferredInputGrad.materialise

    def spy_init(self, *a):
        seen["made"] += 1
        init(self, *a)

    def spy_mat(self):
        seen["formed"] += self._array is None
        return mat(self)
    monkeypatch.setattr(_common.DeferredInputGrad, "__init__", spy_init)
    monkeypatch.setattr(_common.DeferredInputGrad, "materialise", spy_mat)
    monkeypatch.setattr(fused.rms_norm, "fuse_bwd_min_rows", 32)
    monkeypatch.setattr(fused.rms_norm, "fold_min_rows", 32)
    monkeypatch.setattr(fused.ffn_swiglu, "epilogue_min_rows", 32)
    monkeypatch.setattr(fused.qkv_attention, "rope_min_rows", 32)
    return seen


def _llama_step(fuse, monkeypatch):
    from pydynet_amd.llm.llama import Llama
    monkeypatch.setattr(fused.rms_norm, "fuse_bwd", fuse)
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
    ids, tgt = rng.integers(0, V, (B, Lq)), rng.integers(0, V, (B, Lq))
    loss = model.loss(ids, tgt)
    loss.backward()
    grads = {n: host(p_.grad) for n, p_ in model.named_parameters() if p_.requires_grad and p_.grad is not None}
    return float(host(loss)), grads


def test_llama_step_with_the_fusion_on_and_off(lowered, monkeypatch):
    l1, g1 = _llama_step(True, monkeypatch)
    assert lowered == {"fused": 2, "made": 2, "formed": 0}, lowered          # the two block norms of the one layer
    l0, g0 = _llama_step(False, monkeypatch)
    assert lowered == {"fused": 2, "made": 2, "formed": 0}, lowered
    assert abs(l1 - l0) <= 1e-6 * abs(l0), (l1, l0)
    assert g1.keys() == g0.keys() and len(g1) >= 10
    for n in g0:
        close(g1[n], g0[n], f"grad {n}")


# ---- hand-built graphs: x0 -> (pre) -> rms_norm -> ffn_swiglu -> sum, with variations ------------------------------------
class _Case:
    def __init__(self, hp, T=64, x_grad=True, wn_grad=True, seed=0):
        rng = np.random.default_rng(seed)
        t = lambda a, rg: pdn.Tensor(a.astype(np.float32), dtype=np.float32, device="hip:0", requires_grad=rg)
        self.x0 = t(rng.standard_normal((T, D)), x_grad)
        self.wn = t(rng.uniform(0.5, 1.5, D), wn_grad)
        self.buf = hp.from_numpy((0.08 * rng.standard_normal((2, D, F))).astype(np.float32))      # gate | up, equally spaced
        self.wg, self.wu = t(np.zeros((D, F)), True), t(np.zeros((D, F)), True)
        self.wg.data, self.wu.data = self.buf[0], self.buf[1]
        self.wd = t(0.08 * rng.standard_normal((F, D)), True)
        self.w2 = t(0.08 * rng.standard_normal((D, D)), True)
        self.c = t(rng.standard_normal((T, D)), False)

    def leaves(self):
        return {"x0": self.x0, "wn": self.wn, "wg": self.wg, "wu": self.wu, "wd": self.wd, "w2": self.w2}


def _run(build, fuse, monkeypatch, hp, backwards=1, **kw):
    monkeypatch.setattr(fused.rms_norm, "fuse_bwd", fuse)
    Graph.clear()
    case = _Case(hp, **kw)
    loss = build(case)
    for i in range(backwards):
        loss.backward(retain_graph=i + 1 < backwards)
    return {n: np.array(host(t.grad)) for n, t in case.leaves().items() if t.requires_grad and t.grad is not None}


def _both(build, lowered, monkeypatch, hp, expect, **kw):
    on = _run(build, True, monkeypatch, hp, **kw)
    assert lowered == expect, lowered
    off = _run(build, False, monkeypatch, hp, **kw)
    assert lowered == expect, lowered
    assert on.keys() == off.keys() and on
    for n in off:
        close(on[n], off[n], f"grad {n}")


def _plain(c):
    n = fused.rms_norm(c.x0 * 1.5, c.wn)
    return (fused.ffn_swiglu(n, c.wg, c.wu, c.wd) * c.c).sum()


def test_plain_chain_takes_the_fused_entry(lowered, monkeypatch, emulated_hip):
    _both(_plain, lowered, monkeypatch, emulated_hip, {"fused": 1, "made": 1, "formed": 0})


def test_second_consumer_created_after_the_fused_node(lowered, monkeypatch, emulated_hip):
    def build(c):
        n = fused.rms_norm(c.x0 * 1.5, c.wn)
        y = fused.ffn_swiglu(n, c.wg, c.wu, c.wd)
        return (y * c.c).sum() + ((n @ c.w2) * c.c).sum()          # walked first: the norm already holds a gradient
    _both(build, lowered, monkeypatch, emulated_hip, {"fused": 0, "made": 0, "formed": 0})


def test_second_consumer_created_before_the_fused_node(lowered, monkeypatch, emulated_hip):
    def build(c):
        n = fused.rms_norm(c.x0 * 1.5, c.wn)
        other = ((n @ c.w2) * c.c).sum()                            # walked after: adds to the unformed gradient
        y = fused.ffn_swiglu(n, c.wg, c.wu, c.wd)
        return (y * c.c).sum() + other
    _both(build, lowered, monkeypatch, emulated_hip, {"fused": 0, "made": 1, "formed": 1})


def test_retain_graph_and_a_second_backward(lowered, monkeypatch, emulated_hip):
    _both(_plain, lowered, monkeypatch, emulated_hip, {"fused": 0, "made": 1, "formed": 1}, backwards=2)


def test_norm_weight_without_gradient(lowered, monkeypatch, emulated_hip):
    _both(_plain, lowered, monkeypatch, emulated_hip, {"fused": 1, "made": 1, "formed": 0}, wn_grad=False)


def test_norm_weight_that_is_not_a_leaf(lowered, monkeypatch, emulated_hip):
    def build(c):
        n = fused.rms_norm(c.x0 * 1.5, c.wn * 2.0)
        return (fused.ffn_swiglu(n, c.wg, c.wu, c.wd) * c.c).sum()
    _both(build, lowered, monkeypatch, emulated_hip, {"fused": 1, "made": 1, "formed": 0})


def test_raw_input_without_gradient(lowered, monkeypatch, emulated_hip):
    def build(c):
        n = fused.rms_norm(c.x0, c.wn)                              # only the norm weight needs a gradient: d(xn) is formed
        return (fused.ffn_swiglu(n, c.wg, c.wu, c.wd) * c.c).sum()
    _both(build, lowered, monkeypatch, emulated_hip, {"fused": 0, "made": 1, "formed": 1}, x_grad=False)


def test_consumer_whose_input_is_not_an_rms_norm(lowered, monkeypatch, emulated_hip):
    def build(c):
        return (fused.ffn_swiglu(c.x0 * 1.5, c.wg, c.wu, c.wd) * c.c).sum()
    _both(build, lowered, monkeypatch, emulated_hip, {"fused": 0, "made": 0, "formed": 0})
