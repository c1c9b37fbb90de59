"""Links of the lazy chains (core/fused/chain.py) that leave their chain EARLY, before the node that would fuse them.

A pending link somebody reads, or that a node consumes before the chain is complete, materialises as the ordinary operator.
Every check here runs one program built from plain operators twice: on hip:0 (float32, the lazy links active) and on the
cpu device in float64 (no links: each operator runs as it is written), and compares the outputs, the values read and
EVERY leaf gradient at 2e-5 of the float64 tensor's largest entry.  Leaf gradients start as zero-filled buffers, so a
gradient that never arrives fails the comparison.  The exits:
  * a read under no_grad(): `.numpy()`, `.data`, `.item()` of a sum;
  * a consumer that is itself deferred (`F.silu`, `nn.RMSNorm` at its folding width, `F.linear` / `nn.Linear`) or not
    (`F.relu`), read only after the rest of the chain was built;
  * two consumers of one link, the deferred one created first or second;
  * an in-place write to the causal mask after it was built (`mask[...] = `, `+=`, `*=`);
  * a read between the RoPE concat and its final reshape;
  * the same program run again on a fresh tape."""
import math
import zlib

import numpy as np
import pytest

import pydynet_amd as pdn
import pydynet_amd.nn as nn
import pydynet_amd.nn.functional as F
from pydynet_amd.core import fused
from pydynet_amd.core.fused import chain
from pydynet_amd.core.tensor import Graph
from tests.conftest import device_variants

B, L, H, HD = 2, 32, 2, 48              # attention (tests/test_attention_chain.py)
RB, RL, RH, RHD = 2, 8, 3, 16           # rotary embedding (tests/test_rope_chain.py)
RMS_W = 288                             # the width at which nn.RMSNorm on the device is a deferred node

READS = ("numpy", "data", "item")
CONSUMERS = ("silu", "relu", "linear", "nn_linear", "deferred_first", "deferred_second")


def _host(a):
    if a is None:
        return None
    return np.asarray(a.get() if hasattr(a, "get") else a, np.float64)


class _Run:
    """One run of a program: leaves and constants from NumPy arrays, float32 on hip:0, float64 on cpu."""

    def __init__(self, dev):
        self.dev = dev
        self.dt = np.float64 if dev == "cpu" else np.float32
        self.leaves, self.values, self.terms = {}, {}, []

    def leaf(self, name, a):
        t = pdn.Tensor(a, dtype=self.dt, device=self.dev, requires_grad=True)
        self.leaves[name] = t
        return t

    def const(self, a):
        return pdn.Tensor(a, dtype=self.dt, device=self.dev)

    def module(self, name, m, params):
        """A module built on the cpu device, its parameters set from `params`, then moved."""
        for p, a in zip(m.parameters(), params):
            p.data[...] = a
        m.to(self.dev)
        for i, p in enumerate(m.parameters()):
            self.leaves[f"{name}.{i}"] = p
        return m

    def exit(self, t, how, tag):
        """Let link `t` leave its chain: read it now, or hang a consumer on it whose sum joins the loss at the end."""
        rng = np.random.default_rng(zlib.crc32(tag.encode()))
        if how == "numpy":
            with pdn.no_grad():
                self.values[tag] = t.numpy()
        elif how == "data":
            with pdn.no_grad():
                self.values[tag] = _host(t.data)
        elif how == "item":
            with pdn.no_grad():
                self.values[tag] = t.sum().item()
        elif how == "silu":
            self.terms.append(F.silu(t))
        elif how == "relu":
            self.terms.append(F.relu(t))
        elif how == "linear":
            w = self.leaf(f"{tag}.w", rng.standard_normal((t.shape[-1], 32)).astype(np.float32) * 0.3)
            b = self.leaf(f"{tag}.b", rng.standard_normal(32).astype(np.float32))
            self.terms.append(F.linear(t, w, b))
        elif how == "nn_linear":
            lin = self.module(tag, nn.Linear(t.shape[-1], 64, dtype=self.dt),
                              (rng.standard_normal((t.shape[-1], 64)) * 0.3, rng.standard_normal(64)))
            self.terms.append(lin(t))
        elif how == "rms_norm":
            norm = self.module(tag, nn.RMSNorm(t.shape[-1], dtype=self.dt), (1 + 0.5 * rng.standard_normal(t.shape[-1]),))
            self.terms.append(norm(t))
        elif how in ("deferred_first", "deferred_second"):
            c = self.const(rng.standard_normal(t.shape).astype(np.float32))
            if how == "deferred_first":
                self.terms += [F.silu(t), t * c]
            else:
                self.terms += [t * c, F.silu(t)]
        else:
            raise AssertionError(how)

    def loss(self, main):
        for i, c in enumerate(self.terms):
            main = main + c.sum() * (0.5 + 0.25 * i)
        return main


class _defer_small:
    """Let the deferred projection and the deferred norm be built at the small shapes of this module."""

    def __enter__(self):
        self.saved = (fused.linear_relu.min_rows, fused.rms_norm.fold_min_rows, fused.linear_cross_entropy.min_rows)
        fused.linear_relu.min_rows, fused.rms_norm.fold_min_rows, fused.linear_cross_entropy.min_rows = 1, 1, 32

    def __exit__(self, *a):
        fused.linear_relu.min_rows, fused.rms_norm.fold_min_rows, fused.linear_cross_entropy.min_rows = self.saved


def _close(got, ref, what, tol=2e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), (what, "non-finite entries")
    if fin.any():
        scale = max(float(np.abs(ref[fin]).max()), 1e-30)
        err = float(np.abs(got[fin] - ref[fin]).max())
        assert err <= tol * scale + 1e-7, (what, err, scale)


def _compare(program, *args, tol=2e-5, **kw):
    """`program(run, *args)` -> (loss, {name: output}) on cpu float64 and on hip:0; every leaf gradient compared."""
    runs = {}
    with _defer_small():
        for dev in ("cpu", "hip:0"):
            Graph.clear()
            r = _Run(dev)
            loss, outs = program(r, *args, **kw)
            loss.backward()
            runs[dev] = (r, float(loss.item()), {k: v.numpy() for k, v in outs.items()})
    (ref, ref_loss, ref_outs), (got, got_loss, got_outs) = runs["cpu"], runs["hip:0"]
    what = (program.__name__,) + args
    _close(got_loss, ref_loss, what + ("loss",), tol)
    for k in ref_outs:
        _close(got_outs[k], ref_outs[k], what + (k,), tol)
    assert set(got.values) == set(ref.values), what
    for k in ref.values:
        _close(got.values[k], ref.values[k], what + (k,), tol)
    assert set(got.leaves) == set(ref.leaves), what
    for name, t in ref.leaves.items():
        if t.grad is None:
            continue
        g = got.leaves[name].grad
        assert g is not None, what + (name, "no gradient")
        _close(_host(g), _host(t.grad), what + (name, "grad"), tol)
    Graph.clear()
    return got


# ---- the attention chain: qk -> scaled -> masked -> probs ------------------------------------------------------------
def _mask(kind, n):
    if kind == "causal":
        return np.triu(np.full((n, n), float("-inf")), k=1)
    if kind == "additive":                             # finite: any consumer may read it
        rng = np.random.default_rng(11)
        return (rng.standard_normal((1, 1, n, n)) * 2.0 - 4.0 * (rng.random((1, 1, n, n)) < 0.3)).astype(np.float32)
    return None


def attention(r, mask_kind, stage, how, dims=(B, L, H, HD), write=None):
    b, n, h, hd = dims
    rng = np.random.default_rng(3)
    q, k, v = (rng.standard_normal((b, n, h, hd)).astype(np.float32) for _ in range(3))
    gout = rng.standard_normal((b, n, h * hd)).astype(np.float32)
    Q, K, V = r.leaf("q", q), r.leaf("k", k), r.leaf("v", v)
    m = _mask(mask_kind, n)
    M = r.const(m) if m is not None else None
    if write is not None:                              # an in-place write to the mask after it was built
        write(M)
    s = Q.transpose(0, 2, 1, 3) @ K.transpose(0, 2, 3, 1)
    if stage == "qk":
        r.exit(s, how, "qk")
    s = s / math.sqrt(hd)
    if stage == "scaled":
        r.exit(s, how, "scaled")
    if M is not None:
        s = s + M
        if stage == "masked":
            r.exit(s, how, "masked")
    p = F.softmax(s, axis=-1)
    if stage == "probs":
        r.exit(p, how, "probs")
    out = (p @ V.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3).reshape(b, n, -1)
    return r.loss((out * r.const(gout)).sum()), {"out": out}


def _attention_cases():
    for mask_kind in ("none", "additive", "causal"):
        stages = ("qk", "scaled") + (("masked",) if mask_kind != "none" else ()) + ("probs",)
        for stage in stages:
            hows = READS + CONSUMERS
            if stage == "masked" and mask_kind == "causal":
                hows = READS + ("relu",)               # (silu, products and projections of -inf are not finite)
            for how in hows:
                yield mask_kind, stage, how


def check_attention_link_exits(dev):
    for mask_kind, stage, how in _attention_cases():
        n0 = fused.attn_link.fused_built
        _compare(attention, mask_kind, stage, how)
        if how in READS or how == "relu" or how == "deferred_second":
            assert fused.attn_link.fused_built == n0, (mask_kind, stage, how)    # the link was needed before the end


def check_attention_link_into_a_deferred_norm(dev):
    """nn.RMSNorm over the keys axis: a deferred node at the folding width (one head, 288 keys)."""
    for stage in ("qk", "scaled", "probs"):
        _compare(attention, "none", stage, "rms_norm", dims=(1, RMS_W, 1, 16))


def check_causal_mask_written_in_place(dev):
    """The mask was recognised as causal when it was built; what counts is what it holds when the chain fuses."""
    rng = np.random.default_rng(5)
    finite = _mask("additive", L)[0, 0]
    bump = rng.standard_normal((L, L)).astype(np.float32)

    def setitem_all(M):
        M[...] = finite

    def setitem_one(M):
        M[3, 9] = 0.0                                   # row 3 now also sees key 9

    def iadd(M):
        M += pdn.Tensor(bump, device=M.device, dtype=M.dtype)

    def imul(M):
        M *= 2.0

    for write in (setitem_all, setitem_one, iadd, imul):
        n0 = fused.attn_link.fused_built
        _compare(attention, "causal", "none", None, write=write)
        assert fused.attn_link.fused_built == n0 + 1, write.__name__              # still one fused node
    for write in (setitem_one, imul):
        M = pdn.Tensor(_mask("causal", L), device=dev, dtype=np.float32)
        assert M._causal_mask
        write(M)
        assert not M._causal_mask, write.__name__                                # written: no longer trusted


# ---- the rotary embedding: pairs -> comp -> prod -> diff / sum -> unsq -> cat -> reshape -----------------------------
ROPE_STAGES = ("pairs", "comp", "prod", "diff", "sum", "unsq", "cat", "final")


def rope(r, stage, how, dims=(RB, RL, RH, RHD), peek_after_cat=None):
    b, n, h, hd = dims
    rng = np.random.default_rng(9)
    x_np = rng.standard_normal((b, n, h, hd)).astype(np.float32)
    ang = rng.standard_normal((n, hd // 2))
    w_np = rng.standard_normal((b, n, h, hd)).astype(np.float32)
    x = r.leaf("x", x_np)
    cos, sin = r.const(np.cos(ang).astype(np.float32)), r.const(np.sin(ang).astype(np.float32))
    links = {}
    xri = links["pairs"] = x.reshape(*(x.shape[:-1] + (-1, 2)))
    if stage == "pairs":
        r.exit(xri, how, "pairs")
    re, im = xri[..., 0], xri[..., 1]
    links["comp"] = re
    if stage == "comp":
        r.exit(re, how, "comp")
    c, s = pdn.unsqueeze(cos, axis=-2), pdn.unsqueeze(sin, axis=-2)
    rc = links["prod"] = re * c
    if stage == "prod":
        r.exit(rc, how, "prod")
    d = links["diff"] = rc - im * s
    if stage == "diff":
        r.exit(d, how, "diff")
    a = links["sum"] = re * s + im * c
    if stage == "sum":
        r.exit(a, how, "sum")
    u_re = links["unsq"] = pdn.unsqueeze(d, -1)
    u_im = pdn.unsqueeze(a, -1)
    if stage == "unsq":
        r.exit(u_re, how, "unsq")
    cat = pdn.concat([u_re, u_im], axis=-1)
    if stage == "cat":
        r.exit(cat, how, "cat")
    if peek_after_cat is not None:
        r.exit(links[peek_after_cat], "numpy", "peek")
    out = cat.reshape(*(cat.shape[:-2] + (-1,)))
    if stage == "final":
        r.exit(out, how, "final")
    return r.loss((out * r.const(w_np)).sum()), {"out": out}


def check_rope_link_exits(dev):
    for stage in ROPE_STAGES:
        for how in READS + CONSUMERS:
            _compare(rope, stage, how)
    # the case of the report: the pairs of x, straight into a deferred activation
    _compare(rope, "pairs", "silu")


def check_rope_link_into_a_deferred_norm(dev):
    """nn.RMSNorm over the half-width axis of the components: a deferred node at the folding width."""
    for stage in ("comp", "prod", "diff", "sum"):
        _compare(rope, stage, "rms_norm", dims=(1, 4, 2, 2 * RMS_W))


def check_rope_read_between_concat_and_reshape(dev):
    for peek in ("pairs", "comp", "prod", "diff", "sum", "unsq"):
        n0 = chain.rope_link.fused_built
        _compare(rope, "none", None, peek_after_cat=peek)
        assert chain.rope_link.fused_built == n0, peek                            # the plain reshape ran


# ---- silu(gate) * up ---------------------------------------------------------------------------------------------------
def swiglu(r, how):
    rng = np.random.default_rng(13)
    g_np, u_np, w_np = (rng.standard_normal((6, 40)).astype(np.float32) for _ in range(3))
    g, u = r.leaf("gate", g_np), r.leaf("up", u_np)
    act = F.silu(g)
    r.exit(act, how, "silu")
    y = act * u
    return r.loss((y * r.const(w_np)).sum()), {"y": y}


def check_swiglu_pending_silu_exits(dev):
    for how in READS + CONSUMERS:
        _compare(swiglu, how)


# ---- Linear -> reshape -> cross entropy --------------------------------------------------------------------------------
CE_B, CE_L, CE_D, CE_V = 2, 32, 288, 320                  # (tests/test_loss_chain.py)


def linear_ce(r, stage, how):
    rng = np.random.default_rng(17)
    h = r.leaf("h", rng.standard_normal((CE_B, CE_L, CE_D)).astype(np.float32))
    tgt = rng.integers(0, CE_V, CE_B * CE_L)
    head = r.module("head", nn.Linear(CE_D, CE_V, dtype=r.dt),
                    (rng.standard_normal((CE_D, CE_V)) * 0.05, rng.standard_normal(CE_V) * 0.1))
    logits = head(h)
    if stage == "logits":
        r.exit(logits, how, "logits")
    flat = logits.reshape(CE_B * CE_L, CE_V)
    if stage == "flat":
        r.exit(flat, how, "flat")
    loss = nn.CrossEntropyLoss()(flat, pdn.Tensor(tgt, dtype=np.int64, device=r.dev))
    return r.loss(loss), {}


def check_linear_cross_entropy_exits(dev):
    for stage in ("logits", "flat"):
        for how in READS + CONSUMERS:
            built = chain.loss_chain.fused_built
            _compare(linear_ce, stage, how)
            if how in READS:
                assert chain.loss_chain.fused_built == built, (stage, how)       # the projection was read: three nodes


# ---- a second backward on a fresh tape after links materialised -----------------------------------------------------
def check_backward_again_on_a_fresh_tape(dev):
    for _ in range(2):
        _compare(attention, "causal", "scaled", "silu")
        _compare(attention, "causal", "probs", "numpy")
        _compare(rope, "pairs", "silu")
        _compare(rope, "none", None, peek_after_cat="diff")


for _check in (check_attention_link_exits, check_attention_link_into_a_deferred_norm, check_causal_mask_written_in_place,
               check_rope_link_exits, check_rope_link_into_a_deferred_norm, check_rope_read_between_concat_and_reshape,
               check_swiglu_pending_silu_exits, check_linear_cross_entropy_exits, check_backward_again_on_a_fresh_tape):
    device_variants(globals(), _check)


@pytest.mark.gpu
def test_attention_exits_at_256_keys_gpu(hip):
    """The kernels behind materialised links at a larger shape: causal, the probabilities read under no_grad() and a
    deferred silu on the scores, against float64."""
    def both(r, *a):
        b, n, h, hd = 2, 256, 2, 48
        rng = np.random.default_rng(21)
        q, k, v = (rng.standard_normal((b, n, h, hd)).astype(np.float32) for _ in range(3))
        gout = rng.standard_normal((b, n, h * hd)).astype(np.float32)
        Q, K, V = r.leaf("q", q), r.leaf("k", k), r.leaf("v", v)
        M = r.const(_mask("causal", n))
        s = Q.transpose(0, 2, 1, 3) @ K.transpose(0, 2, 3, 1) / math.sqrt(hd)
        r.exit(s, "silu", "scores")
        s = s + M
        p = F.softmax(s, axis=-1)
        r.exit(p, "numpy", "probs")
        out = (p @ V.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3).reshape(b, n, -1)
        return r.loss((out * r.const(gout)).sum()), {"out": out}
    both.__name__ = "attention_256"
    _compare(both)
