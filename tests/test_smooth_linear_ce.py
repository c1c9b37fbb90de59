"""label_smoothing and z_loss on the lm_head + loss node (fused.linear_cross_entropy; the pdnz_ entries of
include/pdn_smoothloss.h around the unchanged products and the unchanged pdnr_linear_ce_backward_rows_f32) against the float64
contract pydynet_amd/core/fused/smooth_loss.py, under tests/test_linear_ce.py's criterion (1e-7 + 1e-4 of the reference's
largest entry).  `cpu` device, emulated C ABI and (``-m gpu``) a real MI355X.

Shapes (rows, V) at D = 288, min_rows = 32, eps = 0.3, lam = 0.05: (64, 96) the smallest supported; (4096, 4000) the
vocabulary cut into ranges by both products and 82 class ranges of the column sums; GPU only (32768, 4000), where the three
split-fp16 forms engage (asserted through pdn_kernel_counters, slots 37 / 39 / 40 and 45), and again with them switched off.
Inputs are tests/test_row_linear_ce.py's `_Problem` WITH x0 + 0.5 and w0 + 0.02: with zero-mean inputs the uniform term
disappears under the tolerance.  Upstream cases: 'normal' -- reduction 'none' under a signed standard normal vector, NaN on
every ignored row; 'mean' -- reduction 'mean', whose gradients are compared AFTER multiplication by 2^20 (exact in float32)
so that `close`'s absolute floor cannot hide them.  Every backward runs TWICE without zero_grad: the leaves must hold twice
the reference.

What the inputs are able to show is asserted from the float64 reference itself: for each of three mutants (uniform term
dropped; one-hot weight left at 1; a_n left at 1) and each of dx, dW and dbias, the mutant differs from the reference by at
least 10 x the tolerance in at least one of the two upstream cases at that shape."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import _lib, nn
from pydynet_amd.core import fused
from pydynet_amd.core.fused import chain, smooth_loss
from pydynet_amd.core.tensor import Graph
from pydynet_amd.optim import Adam
from tests.conftest import device_variants
from tests.test_linear_ce import RT, close, host
from tests.test_masked_linear_ce import FORMS, MASKS, _with

D = 288
EPS, LAM = 0.3, 0.05
UPS = ("normal", "mean")
SCALE = {"normal": 1.0, "mean": 2.0 ** 20}


class _Problem:
    """inputs of one (rows, V, ignore_index), the float64 logits and the references, formed once and shared by its cases"""
    _cache = {}

    def __new__(cls, rows, V, ignore_index, targets=None):
        key = (rows, V, ignore_index, targets)
        if key not in cls._cache:
            cls._cache.clear()                            # (one at a time: the large one holds a GB of float64)
            p = cls._cache[key] = object.__new__(cls)
            rng = np.random.default_rng(rows + V)
            p.rows, p.V, p.ignore_index = rows, V, ignore_index
            p.x0 = (rng.standard_normal((rows, D)) + 0.5).astype(np.float32)
            p.w0 = (0.05 * rng.standard_normal((D, V)) + 0.02).astype(np.float32)
            p.b0 = (0.1 * rng.standard_normal(V)).astype(np.float32)
            p.t0 = rng.integers(1 if ignore_index == 0 else 0, V, rows)
            p.t0[1:4] = (1, V - 1, V // 2)
            p.masks = {"none": np.zeros(rows, bool), "half": rng.random(rows) < 0.5, "row 0": np.arange(rows) == 0,
                       "last row": np.arange(rows) == rows - 1, "all": np.ones(rows, bool)}
            p.u = rng.standard_normal(rows).astype(np.float32)
            if targets == "one class":                    # skew: every valid row shares one target ...
                p.t0[:] = V // 3
            elif targets == "two classes":                # ... or the targets use only the first and the last class
                p.t0[:] = np.where(rng.random(rows) < 0.5, 0, V - 1)
            p.x64, p.w64 = p.x0.astype(np.float64), p.w0.astype(np.float64)
            p.z = p.x64 @ p.w64 + p.b0
            p.refs = {}
        return cls._cache[key]

    def targets(self, mask):
        return self.t0 if self.ignore_index is None else np.where(self.masks[mask], self.ignore_index, self.t0)

    def ignored(self, mask):
        return np.zeros(self.rows, bool) if self.ignore_index is None else self.masks[mask]

    def upstream64(self, mask, up):
        """the float64 upstream number of every row (0 on ignored ones) of ONE backward"""
        keep = ~self.ignored(mask)
        if up == "normal":
            return np.where(keep, self.u.astype(np.float64), 0.0)
        count = int(keep.sum())
        return np.where(keep, 1.0 / count if count else 0.0, 0.0)

    def reference(self, mask, up):
        """(value, dx, dW, dbias) of ONE backward in float64, from smooth_loss.py on the float64 logits"""
        if (mask, up) not in self.refs:
            t = self.targets(mask)
            d = smooth_loss.dlogits(self.z, t, self.upstream64(mask, up), EPS, LAM, self.ignore_index)
            value = smooth_loss.value(self.z, t, EPS, LAM, self.ignore_index, "none" if up == "normal" else "mean")
            self.refs[mask, up] = (np.asarray(value), d @ self.w64.T, self.x64.T @ d, d.sum(0))
        return self.refs[mask, up]

    def mutant_ratios(self, mask):
        """for each mutant and each of dx, dW, dbias: the largest |mutant - reference| / tolerance over the upstream cases,
        both after the two backward passes and the scaling the comparison applies.  The mutants differ from the reference
        by closed forms: +e_n in every column; -u_n eps at the target; -u_n 2 lam lse_n softmax(z_n)."""
        t = self.targets(mask)
        keep = ~self.ignored(mask)
        ts = np.where(keep, t, 0)
        lse = smooth_loss._lse(self.z)
        p = np.exp(self.z - lse[:, None])
        pw = p @ self.w64.T
        wsum = self.w64.sum(1)
        best = {}
        for up in UPS:
            u = self.upstream64(mask, up)
            ref = self.reference(mask, up)
            tol = [1e-7 + RT * float(np.abs(2.0 * SCALE[up] * r).max()) for r in ref[1:]]
            e, ue, ul = u * EPS / self.V, u * EPS, u * 2.0 * LAM * lse
            col = np.zeros((self.V, D))
            np.add.at(col, ts, ue[:, None] * self.x64)
            deltas = {
                "uniform term dropped": (e[:, None] * wsum[None, :], (e[:, None] * self.x64).sum(0), np.array(e.sum())),
                "one-hot weight left at 1": (ue[:, None] * self.w64[:, ts].T, col, np.bincount(ts, weights=ue, minlength=self.V)),
                "a_n left at 1": (ul[:, None] * pw, (self.x64 * ul[:, None]).T @ p, (ul[:, None] * p).sum(0))}
            for name, ds in deltas.items():
                for g, dlt, tl in zip(("dx", "dW", "db"), ds, tol):
                    r = 2.0 * SCALE[up] * float(np.abs(dlt).max()) / tl
                    best[name, g] = max(best.get((name, g), 0.0), r)
        return best


def _assert_mutants_show(p, mask="half"):
    ratios = p.mutant_ratios(mask)
    print(f"({p.rows}, {p.V}) mutant / tolerance:", {k: round(v, 1) for k, v in ratios.items()})
    assert len(ratios) == 9 and min(ratios.values()) >= 10.0, ratios


def _extend():
    from tests.abi_emulator import _loss, _rowloss, _smoothloss
    _loss.extend()
    _rowloss.extend()
    _smoothloss.extend()                                  # (under the emulator: the pdnz_ entries of include/pdn_smoothloss.h)


def _head(dev, p, bias):
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
    return head


def _twice(dev, p, mask, up, plain_operators=False, bias="leaf", passes=2):
    """the value and the gradients after `passes` forward + backward passes without zero_grad in between"""
    Graph.clear()
    head = _head(dev, p, bias)
    x = pdn.Tensor(p.x0, dtype=np.float32, device=dev, requires_grad=True)
    t = pdn.Tensor(p.targets(mask), dtype=np.int64, device=dev)
    u = pdn.Tensor(np.where(p.ignored(mask), np.float32(np.nan), p.u), dtype=np.float32, device=dev)      # NaN on ignored rows
    b = head.bias if bias != "absent" else None
    reduction = "none" if up == "normal" else "mean"
    for _ in range(passes):
        h = x * 1.0                                       # a non-leaf input, as the final norm of the model is
        if plain_operators:
            built, relu_rows = chain.loss_chain.fused_built, fused.linear_relu.min_rows
            fused.linear_relu.min_rows = 1                # (as tests/test_loss_chain.py: the projection stays pending at any row count)
            try:
                crit = nn.CrossEntropyLoss(reduction, p.ignore_index, label_smoothing=EPS, z_loss=LAM)
                out = crit(head(h.reshape(2, p.rows // 2, D)).reshape(p.rows, p.V), t)
            finally:
                fused.linear_relu.min_rows = relu_rows
            assert chain.loss_chain.fused_built == built + 1
        else:
            assert dev == "cpu" or fused.linear_cross_entropy.applicable(h, head.weight, b, t, reduction, p.ignore_index, EPS, LAM)
            out = fused.linear_cross_entropy(h, head.weight, b, t, reduction, p.ignore_index, EPS, LAM)
        assert type(out) is fused.linear_cross_entropy and out.reduction == reduction and out.smooth
        assert (out.label_smoothing, out.z_loss) == (EPS, LAM)
        ((out * u).sum() if up == "normal" else out).backward()
    return (host(out), host(x.grad), host(head.weight.grad),
            host(head.bias.grad) if bias == "leaf" else np.zeros(p.V, np.float32))


def _check(got, ref, ignored, up, what, bias=True, passes=2.0):
    scale = np.float32(SCALE[up])
    grads = [g * scale for g in got[1:]]
    refs = [passes * SCALE[up] * r for r in ref[1:]]
    print(f"{what}: value err {float(np.abs(got[0] - ref[0]).max()):.3e} of {float(np.abs(ref[0]).max()):.3e}", *(
        f"{n} err {float(np.abs(g - r).max()):.3e} of {float(np.abs(r).max()):.3e}"
        for n, g, r in zip(("dx", "dW", "db"), grads, refs)))
    close(np.asarray(got[0]).reshape(ref[0].shape), ref[0], what + ": value")
    for name, g, r in list(zip(("dx", "dW", "db"), grads, refs))[:3 if bias else 2]:
        close(g, r, f"{what}: {name} ({passes:g} backward passes)")
    assert not got[1][ignored].any(), what + ": dx rows of ignored tokens are exactly 0"
    if up == "normal":
        assert not got[0][ignored].any(), what + ": rows of ignored tokens are exactly 0"
    if ignored.all():
        assert all(np.isfinite(g).all() and not g.any() for g in got), what + ": no row left: value and every gradient exactly 0"


def _run(dev, rows, V, ignore_index, cases):
    _extend()
    p = _Problem(rows, V, ignore_index)
    for mask, up in cases:
        what = f"{dev} ({rows}, {V}) ignore_index {ignore_index} {mask} {up}"
        got = _twice(dev, p, mask, up)
        _check(got, p.reference(mask, up), p.ignored(mask), up, what)
        if mask == "half":                                # nn.Linear -> reshape -> CrossEntropyLoss(label_smoothing=, z_loss=): the same node
            ops = _twice(dev, p, mask, up, plain_operators=True)
            _check(ops, p.reference(mask, up), p.ignored(mask), up, what + " plain operators")
            for name, g, o in zip(("value", "dx", "dW", "db"), got, ops):
                close(o, g, f"plain operators: {name} against the node by name")


SMALL = [(m, "normal") for m in MASKS] + [("half", "mean"), ("none", "mean"), ("all", "mean")]
UNMASKED = [("none", u) for u in UPS]
RANGES = [(m, "normal") for m in MASKS] + [("half", "mean")]


@pytest.mark.parametrize("rows,V", [(64, 96), (4096, 4000)])
def test_inputs_tell_the_mutants_apart(rows, V):
    _assert_mutants_show(_Problem(rows, V, -100))


@pytest.mark.parametrize("ignore_index", [-100, 0, None])
def test_smooth_linear_ce_smallest_emulated(emulated_hip, ignore_index):
    _run("hip:0", 64, 96, ignore_index, SMALL if ignore_index is not None else UNMASKED)


@pytest.mark.parametrize("case", RANGES, ids=lambda c: "-".join(c).replace(" ", "_"))
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_smooth_linear_ce_vocabulary_ranges_emulated(emulated_hip, ignore_index, case):
    _run("hip:0", 4096, 4000, ignore_index, [case])


@pytest.mark.parametrize("ignore_index", [-100, None])
def test_smooth_linear_ce_cpu_device(ignore_index):
    """the NumPy-device path of the node: the same contract"""
    p = _Problem(64, 96, ignore_index)
    for mask, up in (SMALL if ignore_index is not None else UNMASKED):
        _check(_twice("cpu", p, mask, up), p.reference(mask, up), p.ignored(mask), up, f"cpu {ignore_index} {mask} {up}")


@pytest.mark.gpu
@pytest.mark.parametrize("ignore_index", [-100, 0, None])
def test_smooth_linear_ce_smallest_gpu(hip, ignore_index):
    _run("hip:0", 64, 96, ignore_index, SMALL if ignore_index is not None else UNMASKED)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RANGES, ids=lambda c: "-".join(c).replace(" ", "_"))
@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_smooth_linear_ce_vocabulary_ranges_gpu(hip, ignore_index, case):
    _run("hip:0", 4096, 4000, ignore_index, [case])


def _forward_form(dev, flags):
    """the three ways the node finds its statistics (both products / the projection's store / a pass over the logits), each
    followed by the new finish; the second and third form dx in the backward pass (the deferred form with the signed
    upstream vector is the vocabulary-ranges test above)"""
    _extend()
    taken, fwd = [], fused.linear_cross_entropy.forward_

    def spy(node, *a):
        out = fwd(node, *a)
        taken.append((node.deferred, node.stats_in_gemm))
        return out
    fused.linear_cross_entropy.forward_ = spy
    try:
        if "lse_epilogue" in flags:       # (no ignore_index: the pass over the logits is then the unmasked forward entry)
            p = _Problem(64, 96, None)
            got_all = _with(flags, lambda: _twice(dev, p, "none", "normal"))
            _check(got_all, p.reference("none", "normal"), np.zeros(64, bool), "normal", f"{dev} {flags} unmasked")
        p = _Problem(4096, 4000, -100)
        got = _with(flags, lambda: _twice(dev, p, "half", "mean"))
        _check(got, p.reference("half", "mean"), p.masks["half"], "mean", f"{dev} {flags} mean")
    finally:
        fused.linear_cross_entropy.forward_ = fwd
    print(flags, "(deferred, stats_in_gemm) =", taken)
    assert taken[0][0] is (not flags)                     # the default is the deferred form at this shape
    assert not (taken[0][1] and "lse_epilogue" in flags)


@pytest.mark.parametrize("flags", FORMS, ids=("deferred", "epilogue_or_pass", "pass"))
def test_smooth_linear_ce_forward_form_emulated(emulated_hip, flags):
    _forward_form("hip:0", flags)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FORMS, ids=("deferred", "epilogue_or_pass", "pass"))
def test_smooth_linear_ce_forward_form_gpu(hip, flags):
    _forward_form("hip:0", flags)


def check_bias_leaf_frozen_absent(dev):
    """a frozen bias and a head without bias: the corrections entry gets no dbias; dx and dW are the reference's either way"""
    _extend()
    L = _lib.lib()
    seen, call = [], L.call

    def spy(name, *a):
        if name.startswith("pdnz_"):
            seen.append((name, a))
        return call(name, *a)
    L.call = spy
    try:
        for bias in ("frozen", "absent", "leaf"):
            p = _Problem(64, 96, -100)
            del seen[:]
            got = _twice(dev, p, "half", "normal", bias=bias)
            names = [n for n, _ in seen]
            assert names == ["pdnz_weight_sums_f32", "pdnz_linear_ce_finish_f32", "pdnz_row_coefficients_f32",
                             "pdnz_linear_ce_corrections_f32"] * 2, names
            for n, a in seen:
                if n == "pdnz_linear_ce_corrections_f32":
                    assert bool(a[9]) is (bias == "leaf") and a[7] and a[8], (bias, a[7:10])
                if n == "pdnz_weight_sums_f32":
                    assert bool(a[1]) is (bias != "absent")
            if bias == "absent":                          # (another problem: logits without p.b0)
                z = p.x64 @ p.w64
                t = p.targets("half")
                d = smooth_loss.dlogits(z, t, p.upstream64("half", "normal"), EPS, LAM, -100)
                ref = (smooth_loss.rows(z, t, EPS, LAM, -100), d @ p.w64.T, p.x64.T @ d, d.sum(0))
                _check(got, ref, p.masks["half"], "normal", f"{dev} bias absent", bias=False)
            else:
                _check(got, p.reference("half", "normal"), p.masks["half"], "normal", f"{dev} bias {bias}", bias=bias == "leaf")
    finally:
        del L.call


def check_skewed_targets(dev):
    """all valid rows share one target (one workgroup of the column sums takes every row); then only classes 0 and V - 1"""
    _extend()
    for targets, up in (("one class", "normal"), ("two classes", "mean")):
        p = _Problem(4096, 4000, -100, targets)
        _check(_twice(dev, p, "half", up), p.reference("half", up), p.masks["half"], up, f"{dev} {targets} {up}")


def check_two_runs_give_the_same_bits(dev):
    """the same backward from zeroed gradients twice: bit-identical dW and dbias (every sum in a fixed order, no atomics)"""
    _extend()
    p = _Problem(4096, 4000, -100)
    a = _twice(dev, p, "half", "normal", passes=1)
    b = _twice(dev, p, "half", "normal", passes=1)
    _check(a, p.reference("half", "normal"), p.masks["half"], "normal", f"{dev} one pass", passes=1.0)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[1], b[1])


for _f in (check_bias_leaf_frozen_absent, check_skewed_targets, check_two_runs_give_the_same_bits):
    device_variants(globals(), _f)


def _counters(reset):
    buf = (ctypes.c_int64 * 46)()
    _lib.lib().call("pdn_kernel_counters", buf, 46, 1 if reset else 0)
    return list(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [True, False])
def test_smooth_linear_ce_split_fp16_forms_gpu(hip, split):
    """32768 rows: the projection (slot 37), the input gradient (slot 39) and the weight gradient (slot 40) on split-fp16 MFMA
    around the pdnr_ backward (slot 44) and the new entries (slot 45: weight sums, finish, coefficients and corrections of
    each of the two passes); with the three switches off the fp32 forms (slots 5, 12, 13 alone)."""
    rows, V = 32768, 4000
    p = _Problem(rows, V, -100)
    if split:
        _assert_mutants_show(p)
    flags = {} if split else {"split_forward": False, "split_dx": False, "split_dw": False}
    for up in UPS:
        _counters(True)
        got = _with(flags, lambda: _twice("hip:0", p, "half", up))
        cnt = _counters(True)
        print("counters 5, 12, 13, 37, 39, 40, 44, 45:", [cnt[i] for i in (5, 12, 13, 37, 39, 40, 44, 45)])
        assert cnt[5] == 2 and cnt[12] == 2 and cnt[13] == 2, cnt
        assert [cnt[37], cnt[39], cnt[40]] == ([2, 2, 2] if split else [0, 0, 0]), cnt
        assert cnt[44] == 2 and cnt[45] == 8, cnt
        _check(got, p.reference("half", up), p.masks["half"], up, f"(32768, 4000) split {split} {up}")


def _trajectory(hip, use_graph):
    """lm_head + smoothed loss -> backward -> Adam over five target buffers, eagerly or replayed from one capture"""
    p = _Problem(64, 96, -100)
    rng = np.random.default_rng(11)
    tgts = rng.integers(0, p.V, (5, p.rows))
    tgts[1][rng.random(p.rows) < 0.5] = -100
    tgts[2][:] = 7                                        # every row the same class
    tgts[3][:] = -100                                     # no row left: a step with zero gradient
    Graph.clear()
    head = _head("hip:0", p, "leaf")
    opt = Adam(head.parameters(), lr=1e-2)
    opt.flatten_grads()
    x = pdn.Tensor(p.x0, dtype=np.float32, device="hip:0", requires_grad=True)
    tgd = pdn.Tensor(tgts[0], dtype=np.int64, device="hip:0")

    def step():
        opt.zero_grad()
        loss = fused.linear_cross_entropy(x * 1.0, head.weight, head.bias, tgd, "mean", -100, EPS, LAM)
        loss.backward()
        opt.step()
        return loss
    losses = []
    if use_graph:
        g = hip.Graph()
        loss = g.capture(step)                            # steps 1 and 2 on the first buffer
        losses.append(loss.item())
        for t in tgts[1:]:
            tgd.data[...] = hip.from_numpy(t)
            g.replay()
            losses.append(loss.item())
        g.destroy()
    else:
        step()
        losses.append(step().item())
        for t in tgts[1:]:
            tgd.data[...] = hip.from_numpy(t)
            losses.append(step().item())
    return losses, {n: q.numpy() for n, q in head.named_parameters()}


@pytest.mark.gpu
def test_replayed_smoothed_steps_follow_the_targets_buffer(hip):
    eager, replayed = _trajectory(hip, False), _trajectory(hip, True)
    print("eager", eager[0], "replayed", replayed[0])
    close(np.array(replayed[0]), np.array(eager[0]), "losses")
    assert eager[0][3] == 0.0 and len(set(np.round(eager[0], 3))) == 5
    for n in eager[1]:
        close(replayed[1][n], eager[1][n], "parameter " + n)
