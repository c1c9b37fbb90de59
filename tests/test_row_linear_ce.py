"""reduction='none' on the lm_head + loss node (fused.linear_cross_entropy; C ABI pdnr_linear_ce_finish_rows_f32 and
pdnr_linear_ce_backward_rows_f32 of include/pdn_rowloss.h around the unchanged products) against the float64 contract
pydynet_amd/core/fused/row_loss.py, under tests/test_linear_ce.py's criterion (1e-7 + 1e-4 of the reference's largest entry).
Emulated C ABI and (``-m gpu``) a real MI355X.

Shapes (rows, V) at D = 288, min_rows = 32: (64, 96) the smallest supported; (4096, 4000) the vocabulary cut into ranges by
both products; GPU only (32768, 4000), the fewest rows at which the split-fp16 forward, dx and dW forms all engage (asserted
through pdn_kernel_counters, with slot 44), and again with the three switched off.  Masks and ignore_index values are
tests/test_masked_cross_entropy.py's.  Every backward runs TWICE without zero_grad: the leaf gradients must hold twice the
reference.  Upstream vectors: signed standard normal; one non-zero row; all zero (every gradient exactly 0, no NaN); the
constant 2^-20, whose gradients are compared AFTER multiplication by 2^20 (exact in float32) against the 'sum' node's
reference -- under `close`'s absolute floor of 1e-7 the unscaled comparison would pass anything; this is the case the
normaliser s = max |u| of the weight gradient exists for.  On every ignored row the upstream vector holds NaN: dx rows of
ignored tokens, and every other gradient, must not see it."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib, nn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import chain, masked_loss, row_loss
from pydynet_amd.core.tensor import Graph
from tests.test_linear_ce import close, host
from tests.test_masked_linear_ce import FORMS, MASKS, _with

D = 288
UPS = ("normal", "one row", "zero", "tiny")
TINY = np.float32(2.0 ** -20)


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
            one = np.zeros(rows, np.float32)
            one[rows // 3] = -1.5
            p.ups = {"normal": rng.standard_normal(rows).astype(np.float32), "one row": one,
                     "zero": np.zeros(rows, np.float32), "tiny": np.full(rows, TINY)}
            p.z = p.x0.astype(np.float64) @ p.w0.astype(np.float64) + p.b0
            p.refs = {}
        return cls._cache[key]

    def targets(self, mask):
        return self.t0 if self.ignore_index is None else np.where(self.masks[mask], self.ignore_index, self.t0)

    def ignored(self, mask):
        return np.zeros(self.rows, bool) if self.ignore_index is None else self.masks[mask]

    def upstream(self, mask, up):
        """the vector handed to the node: NaN wherever the row is ignored"""
        return np.where(self.ignored(mask), np.float32(np.nan), self.ups[up])

    def reference(self, mask, up):
        """(rows, dx, dW, dbias) of ONE backward, float64; for 'tiny' the 'sum' node's reference (upstream 1): the test
        multiplies what it got by 2^20 first"""
        if (mask, up) not in self.refs:
            t = self.targets(mask)
            if up == "tiny":
                d = masked_loss.cross_entropy(self.z, t, -100 if self.ignore_index is None else self.ignore_index, "sum", 1.0)[1]
            else:
                d = row_loss.dlogits(self.z, t, self.ups[up], self.ignore_index)
            self.refs[mask, up] = (row_loss.rows(self.z, t, self.ignore_index), d @ self.w0.astype(np.float64).T,
                                   self.x0.astype(np.float64).T @ d, d.sum(0))
        return self.refs[mask, up]


def _extend():
    from tests.abi_emulator import _loss, _rowloss
    _loss.extend()
    _rowloss.extend()                                     # (under the emulator: the pdnr_ entries of include/pdn_rowloss.h)


def _twice(dev, p, mask, up, plain_operators=False, bias="leaf"):
    """the rows and the gradients after TWO forward + backward passes without zero_grad in between"""
    Graph.clear()
    fused.linear_cross_entropy.min_rows = 32              # (as tests/test_linear_ce.py: the model takes the node from 32768 tokens up)
    head = nn.Linear(D, p.V, bias=bias != "absent", dtype=np.float32)
    head.weight.data[...] = p.w0
    if bias != "absent":
        head.bias.data[...] = p.b0
    head.to(dev)
    head.weight.zero_grad()
    if bias == "leaf":
        head.bias.zero_grad()
    elif bias == "frozen":
        head.bias.requires_grad = False
    x = pdn.Tensor(p.x0, dtype=np.float32, device=dev, requires_grad=True)
    t = pdn.Tensor(p.targets(mask), dtype=np.int64, device=dev)
    u = pdn.Tensor(p.upstream(mask, up), dtype=np.float32, device=dev)
    b = head.bias if bias != "absent" else None
    for _ in range(2):
        h = x * 1.0                                       # a non-leaf input, as the final norm of the model is
        if plain_operators:
            built, relu_rows = chain.loss_chain.fused_built, fused.linear_relu.min_rows
            fused.linear_relu.min_rows = 1                # (as tests/test_loss_chain.py: the projection stays pending at any row count)
            try:
                per_row = nn.CrossEntropyLoss("none", p.ignore_index)(head(h.reshape(2, p.rows // 2, D)).reshape(p.rows, p.V), t)
            finally:
                fused.linear_relu.min_rows = relu_rows
            assert chain.loss_chain.fused_built == built + 1
        else:
            assert dev == "cpu" or fused.linear_cross_entropy.applicable(h, head.weight, b, t, "none", p.ignore_index)
            per_row = fused.linear_cross_entropy(h, head.weight, b, t, "none", p.ignore_index)
        assert type(per_row) is fused.linear_cross_entropy and per_row.reduction == "none" and per_row.shape == (p.rows,)
        (per_row * u).sum().backward()
    return (host(per_row), host(x.grad), host(head.weight.grad),
            host(head.bias.grad) if bias == "leaf" else np.zeros(p.V, np.float32))


def _check(got, ref, ignored, up, what, bias=True):
    scale = np.float32(2.0 ** 20) if up == "tiny" else np.float32(1)
    grads = [g * scale for g in got[1:]]
    print(f"{what}: rows err {float(np.abs(got[0] - ref[0]).max()):.3e} of {float(np.abs(ref[0]).max()):.3e}", *(
        f"{n} err {float(np.abs(g - 2.0 * r).max()):.3e} of {float(np.abs(2.0 * r).max()):.3e}"
        for n, g, r in zip(("dx", "dW", "db"), grads, ref[1:])))
    close(got[0], ref[0], what + ": rows")
    for name, g, r in list(zip(("dx", "dW", "db"), grads, ref[1:]))[:3 if bias else 2]:
        close(g, 2.0 * r, f"{what}: {name} (two backward passes)")
    assert not got[0][ignored].any() and not got[1][ignored].any(), what + ": rows and dx rows of ignored tokens are exactly 0"
    if up == "zero" or ignored.all():
        assert all(np.isfinite(g).all() and not g.any() for g in got[1:]), what + ": every gradient exactly 0"


def _run(dev, rows, V, ignore_index, cases):
    _extend()
    p = _Problem(rows, V, ignore_index)
    for mask, up in cases:
        what = f"{dev} ({rows}, {V}) ignore_index {ignore_index} {mask} u {up}"
        got = _twice(dev, p, mask, up)
        _check(got, p.reference(mask, up), p.ignored(mask), up, what)
        if mask == "half" and up == "normal":             # nn.Linear -> reshape -> CrossEntropyLoss('none'): the same node
            ops = _twice(dev, p, mask, up, plain_operators=True)
            _check(ops, p.reference(mask, up), p.ignored(mask), up, what + " plain operators")
            for name, g, o in zip(("rows", "dx", "dW", "db"), got, ops):
                close(o, g, f"plain operators: {name} against the node by name")


SMALL = [(m, "normal") for m in MASKS] + [("half", u) for u in UPS[1:]] + [("none", "tiny")]
RANGES = [(m, "normal") for m in MASKS] + [("half", u) for u in UPS[1:]]


@pytest.mark.parametrize("ignore_index", [-100, 0, None])
def test_row_linear_ce_smallest_emulated(emulated_hip, ignore_index):
    _run("hip:0", 64, 96, ignore_index, SMALL if ignore_index is not None else [("none", u) for u in UPS])


@pytest.mark.parametrize("case", RANGES, ids=lambda c: "-".join(c).replace(" ", "_"))
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_row_linear_ce_vocabulary_ranges_emulated(emulated_hip, ignore_index, case):
    _run("hip:0", 4096, 4000, ignore_index, [case])


@pytest.mark.parametrize("ignore_index", [-100, None])
def test_row_linear_ce_cpu_device(ignore_index):
    """the NumPy-device path of the node: the same contract"""
    p = _Problem(64, 96, ignore_index)
    for mask, up in (SMALL if ignore_index is not None else [("none", u) for u in UPS]):
        _check(_twice("cpu", p, mask, up), p.reference(mask, up), p.ignored(mask), up, f"cpu {ignore_index} {mask} {up}")


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_index", [-100, 0, None])
def test_row_linear_ce_smallest_gpu(hip, ignore_index):
    _run("hip:0", 64, 96, ignore_index, SMALL if ignore_index is not None else [("none", u) for u in UPS])


@pytest.mark.gpu
@pytest.mark.parametrize("case", RANGES, ids=lambda c: "-".join(c).replace(" ", "_"))
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_row_linear_ce_vocabulary_ranges_gpu(hip, ignore_index, case):
    _run("hip:0", 4096, 4000, ignore_index, [case])


def _forward_form(dev, flags):
    """the three ways the node finds its statistics (both products / the projection's store / a pass over the logits), each
    followed by the row finish; the second and third form dx in the backward pass"""
    _extend()
    p = _Problem(4096, 4000, -100)
    taken, fwd = [], fused.linear_cross_entropy.forward_

    def spy(node, *a):
        out = fwd(node, *a)
        taken.append((node.deferred, node.stats_in_gemm))
        return out
    fused.linear_cross_entropy.forward_ = spy
    try:
        got = _with(flags, lambda: _twice(dev, p, "half", "normal"))
        # (no ignore_index: the pass over the logits is then the unmasked forward entry, followed by the same finish)
        got_all = _with(flags, lambda: _twice(dev, _Problem(4096, 4000, None), "none", "normal")) if "lse_epilogue" in flags else None
    finally:
        fused.linear_cross_entropy.forward_ = fwd
    print(flags, "(deferred, stats_in_gemm) =", taken)
    assert taken[0][0] is (not flags)                     # the default is the deferred form at this shape
    assert not (taken[0][1] and "lse_epilogue" in flags)
    if got_all is not None:
        _check(got_all, _Problem(4096, 4000, None).reference("none", "normal"), np.zeros(4096, bool), "normal", f"{dev} {flags} unmasked")
    p = _Problem(4096, 4000, -100)
    _check(got, p.reference("half", "normal"), p.masks["half"], "normal", f"{dev} {flags}")


@pytest.mark.parametrize("flags", FORMS, ids=("deferred", "epilogue_or_pass", "pass"))
def test_row_linear_ce_forward_form_emulated(emulated_hip, flags):
    _forward_form("hip:0", flags)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FORMS, ids=("deferred", "epilogue_or_pass", "pass"))
def test_row_linear_ce_forward_form_gpu(hip, flags):
    _forward_form("hip:0", flags)


def _no_colsum_without_bias_gradient(dev):
    """a frozen bias, and a head without bias, launch no column-sum kernel: the backward entry gets no dbias and no column-sum
    workspace, and the entry of the pass on its own is not called either; a bias that needs its gradient gets both"""
    _extend()
    p = _Problem(64, 96, -100)
    L = _lib.lib()
    seen, call = [], L.call

    def spy(name, *a):
        if name.startswith("pdnr_"):
            seen.append((name, a))
        return call(name, *a)
    L.call = spy
    try:
        for bias in ("frozen", "absent", "leaf"):
            del seen[:]
            got = _twice(dev, p, "half", "normal", bias=bias)
            names = [n for n, _ in seen]
            assert names.count("pdnr_linear_ce_backward_rows_f32") == 2 and "pdnr_weighted_colsum_f32" not in names, names
            for n, a in seen:
                if n == "pdnr_linear_ce_backward_rows_f32":
                    dbias, cws, cwsb = a[11], a[20], a[21]
                    assert (bool(dbias), bool(cws), cwsb > 0) == ((True,) * 3 if bias == "leaf" else (False,) * 3), (bias, dbias, cws, cwsb)
            if bias == "absent":                          # (the reference's logits carry p.b0: another problem, dW checked below)
                continue
            _check(got, p.reference("half", "normal"), p.masks["half"], "normal", f"{dev} bias {bias}", bias=bias == "leaf")
    finally:
        del L.call


def test_no_colsum_without_bias_gradient_emulated(emulated_hip):
    _no_colsum_without_bias_gradient("hip:0")


@pytest.mark.gpu
def test_no_colsum_without_bias_gradient_gpu(hip):
    _no_colsum_without_bias_gradient("hip:0")


def _counters(reset):
    buf = (ctypes.c_int64 * 45)()
    _lib.lib().call("pdn_kernel_counters", buf, 45, 1 if reset else 0)
    return list(buf)


def _weighted_colsum_entry(dev):
    """pdnr_weighted_colsum_f32 and pdnr_scale_rows_f32 / pdnr_abs_max_rows_f32 called on their own: odd sizes (no float4), an
    accumulating db_beta, more than one row slab, a strided input"""
    from pydynet_amd import hipnp as hp
    _extend()
    L = _lib.lib()
    rng = np.random.default_rng(5)
    for rows, V in ((70, 10), (4100, 1028)):
        z = (2.0 * rng.standard_normal((rows, V))).astype(np.float32)
        t = rng.integers(0, V, rows)
        t[rng.random(rows) < 0.3] = V                     # targets_safe: V marks an ignored row
        keep = t != V
        lse = np.where(keep, np.log(np.exp(z.astype(np.float64)).sum(-1)), np.inf).astype(np.float32)
        u = np.where(keep, rng.standard_normal(rows), np.nan).astype(np.float32)
        b0 = rng.standard_normal(V).astype(np.float32)
        ref = 0.5 * b0 + row_loss.dlogits(z, np.where(keep, t, -1), u, -1).sum(0)
        zd, td, ld, ud, bd = (hp.from_numpy(a) for a in (z, t.astype(np.int64), lse, u, b0))
        need = L.query("pdnr_weighted_colsum_workspace_bytes", rows, V)
        assert need >= V * 4
        ws, wsb = hp.workspace(need)
        _counters(True)
        L.call("pdnr_weighted_colsum_f32", zd._ptr, V, ld._ptr, td._ptr, ud._ptr, rows, V, bd._ptr, 0.5, ws, wsb, hp.stream())
        close(bd, ref, f"({rows}, {V}) weighted column sums")
        with pytest.raises(_lib.HipLibraryError):
            L.call("pdnr_weighted_colsum_f32", zd._ptr, V, ld._ptr, td._ptr, ud._ptr, rows, V, bd._ptr, 0.5, ws, need - 4, hp.stream())
        s_dev = hp.empty((2,), np.float32)
        L.call("pdnr_abs_max_rows_f32", ud._ptr, td._ptr, V, rows, s_dev._ptr, hp.stream())
        s, inv = row_loss.abs_max(u, keep)
        got_s = host(s_dev)
        assert got_s[0] == np.float32(s) and abs(got_s[1] - inv) <= 1e-6 * inv
        out = hp.empty((rows, V - 1), np.float32)          # a strided input (V - 1 of V columns), an odd width
        L.call("pdnr_scale_rows_f32", zd._ptr, V, out._ptr, V - 1, rows, V - 1, ud._ptr, s_dev._ptr + 4, td._ptr, V, hp.stream())
        ref_s = row_loss.scale_rows(z[:, :V - 1], u, keep, float(got_s[1]))
        close(out, ref_s, f"({rows}, {V}) scaled rows")
        assert not host(out)[~keep].any()
        L.call("pdnr_scale_rows_f32", zd._ptr, V, zd._ptr, V, rows, V, ud._ptr, None, td._ptr, V, hp.stream())      # in place
        close(zd, row_loss.scale_rows(z, u, keep), f"({rows}, {V}) rows scaled in place")
        assert _counters(True)[44] == 5                   # once per entry (the call refused for its workspace included)
    # all rows ignored / all weights zero: s = 0 and 1 / s = 0
    td = hp.from_numpy(np.full(8, 3, np.int64))
    s_dev = hp.empty((2,), np.float32)
    L.call("pdnr_abs_max_rows_f32", hp.from_numpy(np.ones(8, np.float32))._ptr, td._ptr, 3, 8, s_dev._ptr, hp.stream())
    assert not host(s_dev).any()


def test_weighted_colsum_entry_emulated(emulated_hip):
    _weighted_colsum_entry("hip:0")


@pytest.mark.gpu
def test_weighted_colsum_entry_gpu(hip):
    _weighted_colsum_entry("hip:0")


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False])
def test_row_linear_ce_split_fp16_forms_gpu(hip, split):
    """32768 rows: the projection (slot 37), the input gradient (slot 39) and the weight gradient (slot 40) on split-fp16 MFMA
    around the row finish and backward (slot 44); with the three switches off the fp32 forms (slots 5, 12, 13 alone).  The
    2^-20 upstream must hold on both: without the normaliser the split-fp16 planes of x * u would be subnormal."""
    rows, V = 32768, 4000
    p = _Problem(rows, V, -100)
    flags = {} if split else {"split_forward": False, "split_dx": False, "split_dw": False}
    _counters(True)
    got = _with(flags, lambda: _twice("hip:0", p, "half", "normal"))
    cnt = _counters(True)
    print("counters 5, 12, 13, 37, 39, 40, 44:", [cnt[i] for i in (5, 12, 13, 37, 39, 40, 44)])
    assert cnt[5] == 2 and cnt[12] == 2 and cnt[13] == 2, cnt
    assert [cnt[37], cnt[39], cnt[40]] == ([2, 2, 2] if split else [0, 0, 0]), cnt
    assert cnt[44] > 0, cnt
    _check(got, p.reference("half", "normal"), p.masks["half"], "normal", f"(32768, 4000) split {split}")
    tiny = _with(flags, lambda: _twice("hip:0", p, "half", "tiny"))
    _check(tiny, p.reference("half", "tiny"), p.masks["half"], "tiny", f"(32768, 4000) split {split} u = 2^-20")
