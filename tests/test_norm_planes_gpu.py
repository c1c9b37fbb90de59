"""include/pdn_normplanes.h on the GPU: the projections that do not write the block norm's output, and the packed weight
gradient whose plane pass forms that output from (x, norm_w, rms) in one launch (stn_split_xn_kernel of
csrc/split_tn_planes.hip), each against what it replaces.

Forward: the new entries against pdn_*_norm_fwd_f32 on the same inputs -- qkv / gu / h / rms bit for bit -- at 16384 rows
(RTS_MIN_ROWS) and at a row count that is no multiple of 256 (the GUARD instantiation): 16384 + 8 for gate | up; q | k | v
needs rows in whole sequences of a multiple of 32 positions, so its ragged count is 16384 + 32 (sequences of 32).  The
outputs of the new call lie in one arena laid out as the old call's, with a canary where xn was and behind every output.

Weight gradient: K = 32768 (OTS_MIN_K) and 32768 + 32 (K ranges of unequal length), blocks 3 x 288 and 2 x 768, beta 0 and 1.
x standard normal with a column at 1e-4 of the others and one norm weight 0; xn and rms come from the existing forward.
Reference: float64 from x, rms, w, G on 64 sampled columns.  Bound: error of the new entry over the reference's largest
entry <= 2 x the same figure of the existing route (pdn_gemm_f32 on the written xn), per block.  The second launch equals
the first bit for bit; with PDN_NORM_PLANES=0 the entry equals the existing route bit for bit; a NaN row of x marks the same
entries in both.  Every case prints its figures; the printout of a run is profiles/norm_planes_gpu_tests.txt.

Node level: one loss.backward() of a two-layer width-288 model at 65536 tokens with the class switch on and off: every
gradient within 1e-4 of the tensor's largest entry (the batch gate's bound), the plane-launch counter at 2 per layer."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, F, HD = 288, 768, 48
CANARY = np.float32(7.5)
_CACHE = {}


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def _bits(a):
    return a.view(np.uint32)


# ---- forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M,seq", [("qkv", 16384, 256), ("qkv", 16384 + 32, 32), ("gu", 16384, 0), ("gu", 16384 + 8, 0)],
                         ids=["qkv_16384", "qkv_16416_guard", "gu_16384", "gu_16392_guard"])
def test_forward_without_xn_equals_the_forward_with_it(hip, kind, M, seq):
    L, hp = _lib_hp()
    rng = np.random.default_rng(M)
    x = hp.from_numpy(rng.standard_normal((M, D), dtype=np.float32) * (10.0 ** rng.uniform(-2, 2, (M, 1))).astype(np.float32))
    wn = hp.from_numpy(rng.uniform(0.5, 1.5, D).astype(np.float32))
    if kind == "qkv":
        assert L.query("pdnp_qkv_rope_norm_supported", M, D, D, seq, HD) == 1
        w = hp.from_numpy(0.05 * rng.standard_normal((3, D, D), dtype=np.float32))
        ang = rng.uniform(0, 6.28, (seq, HD)).astype(np.float32)
        tab = hp.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], -1).astype(np.float32))
        sizes = {"rms": M, "xn": M * D, "out": M * 3 * D}
    else:
        assert L.query("pdnp_gateup_swiglu_norm_supported", M, F, D) == 1
        w = hp.from_numpy(0.05 * rng.standard_normal((2, D, F), dtype=np.float32))
        sizes = {"rms": M, "xn": M * D, "out": M * 2 * F, "h": M * F}
    pad = 64                                                   # floats of canary behind every part (keeps 16-byte alignment)
    offs, pos = {}, 0
    for name, n in sizes.items():
        offs[name] = pos
        pos += (n + 3) // 4 * 4 + pad
    arenas = [hp.from_numpy(np.full(pos, CANARY, np.float32)) for _ in range(2)]
    ptr = lambda a, name: a._ptr + 4 * offs[name]
    for new, a in ((False, arenas[0]), (True, arenas[1])):
        xn_arg = () if new else (ptr(a, "xn"),)
        if kind == "qkv":
            L.call("pdnp_qkv_rope_norm_fwd_f32" if new else "pdn_qkv_rope_norm_fwd_f32", x._ptr, wn._ptr, 1e-6, *xn_arg,
                   ptr(a, "rms"), w._ptr, D * D, ptr(a, "out"), tab._ptr, M, D, D, seq, HD, D, hp.stream())
        else:
            L.call("pdnp_gateup_swiglu_norm_fwd_f32" if new else "pdn_gateup_swiglu_norm_fwd_f32", x._ptr, wn._ptr, 1e-6, *xn_arg,
                   ptr(a, "rms"), w._ptr, D * F, ptr(a, "out"), ptr(a, "h"), M, F, D, D, hp.stream())
    old, got = arenas[0].get(), arenas[1].get()
    for name, n in sizes.items():
        o = offs[name]
        if name == "xn":
            assert np.all(got[o:o + n] == CANARY), "the place of xn was written"
            assert not np.any(old[o:o + n] == CANARY)
        else:
            assert np.array_equal(_bits(got[o:o + n]), _bits(old[o:o + n])), f"{name} differs"
        end = o + (n + 3) // 4 * 4 + pad
        assert np.all(got[o + n:end] == CANARY) and np.all(old[o + n:end] == CANARY), f"written behind {name}"


# ---- weight gradient ------------------------------------------------------------------------------------------------------
class _Problem:
    """one (K, block shape): x, norm weight, G; xn and rms from the existing forward; the float64 reference on 64 columns"""

    def __init__(self, K, nbc, nb):
        L, hp = _lib_hp()
        self.L, self.hp, self.K, self.nbc, self.nb = L, hp, K, nbc, nb
        rng = np.random.default_rng(K + nbc)
        x = rng.standard_normal((K, D), dtype=np.float32)
        x[:, 5] *= np.float32(1e-4)                          # a column far below its row's rms
        w = rng.uniform(0.5, 1.5, D).astype(np.float32)
        w[7] = 0.0
        w[11] = -w[11]
        self.g = 1e-3 * rng.standard_normal((K, nb * nbc), dtype=np.float32)
        self.dw0 = rng.standard_normal((nb, D, nbc), dtype=np.float32)
        self.xd, self.wd, self.gd = hp.from_numpy(x), hp.from_numpy(w), hp.from_numpy(self.g)
        self.gb = hp.ndarray(self.gd._buf, self.gd._ptr, (nb, K, nbc), (nbc, nb * nbc, 1), self.gd.dtype)
        self.xn, self.rms = self.forward(self.xd)
        self.cols = np.sort(rng.choice(nb * nbc, 64, replace=False))
        xn64 = x.astype(np.float64) / self.rms.get().astype(np.float64)[:, None] * w.astype(np.float64)
        self.ref = xn64.T @ self.g[:, self.cols].astype(np.float64)                     # (288, 64)
        self.x = x
        self.nbytes = L.query("pdnp_norm_dw_blocks_workspace_bytes", K, nbc, nb)
        with _env("PDN_NORM_PLANES", "0"):
            self.nbytes = max(self.nbytes, L.query("pdnp_norm_dw_blocks_workspace_bytes", K, nbc, nb))
        self.ws = hp.empty((self.nbytes,), np.bool_)

    def forward(self, xd):
        """xn and rms as the existing gate | up forward leaves them (any row count from 16384 on)"""
        L, hp, K = self.L, self.hp, self.K
        wgu = hp.zeros((2, D, F), np.float32)
        xn, rms = hp.empty((K, D), np.float32), hp.empty((K,), np.float32)
        gu, h = hp.empty((K, 2 * F), np.float32), hp.empty((K, F), np.float32)
        L.call("pdn_gateup_swiglu_norm_fwd_f32", xd._ptr, self.wd._ptr, 1e-6, xn._ptr, rms._ptr, wgu._ptr, D * F, gu._ptr, h._ptr,
               K, F, D, D, hp.stream())
        return xn, rms

    def existing(self, beta, xn=None):
        dw = self.hp.from_numpy(self.dw0)
        self.hp.gemm((xn if xn is not None else self.xn).T, self.gb, dw, beta=beta)
        return dw.get()

    def entry(self, beta, xd=None, rms=None):
        dw = self.hp.from_numpy(self.dw0)
        self.L.call("pdnp_norm_dw_blocks_f32", (xd if xd is not None else self.xd)._ptr, self.wd._ptr, (rms if rms is not None else self.rms)._ptr, self.gd._ptr,
                    self.nb * self.nbc, dw._ptr, D * self.nbc, beta, self.K, self.nbc, self.nb, self.ws._ptr, self.nbytes,
                    self.hp.stream())
        return dw.get()

    def errors(self, dw, beta):
        """per block: largest error on the sampled columns over the reference's largest entry there"""
        out = []
        for b in range(self.nb):
            sel = (self.cols >= b * self.nbc) & (self.cols < (b + 1) * self.nbc)
            c = self.cols[sel] - b * self.nbc
            ref = self.ref[:, sel] + beta * self.dw0[b][:, c]
            out.append(float(np.abs(dw[b][:, c] - ref).max()) / float(np.abs(ref).max()))
        return out


def _problem(key):
    if key not in _CACHE:
        _CACHE.clear()                       # one shape's arrays at a time
        _CACHE[key] = _Problem(*key)
    return _CACHE[key]


def _launches(L):
    return L.query("pdnp_norm_dw_blocks_plane_launches", 0)


SHAPES = [(32768, 288, 3), (32768 + 32, 288, 3), (32768, 768, 2), (32768 + 32, 768, 2)]


@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"K{s[0]}_{s[2]}x{s[1]}")
def test_weight_gradient_against_float64_and_the_existing_route(hip, shape, beta):
    P = _problem(shape)
    n0 = _launches(P.L)
    new = P.entry(beta)
    assert _launches(P.L) - n0 == 1
    again = P.entry(beta)
    assert np.array_equal(_bits(new), _bits(again)), "two launches differ"
    old = P.existing(beta)
    e_n, e_o = P.errors(new, beta), P.errors(old, beta)
    line = f"K={P.K} blocks {P.nb} x {P.nbc} beta={beta:g}: new " + " ".join(f"{e:.3e}" for e in e_n) + \
           "; existing " + " ".join(f"{e:.3e}" for e in e_o)
    print(line)
    assert np.all(np.isfinite(new))
    assert not new[:, 7, :].any() or beta != 0.0             # the row of dW of a zero norm weight is exactly zero
    for a, b in zip(e_n, e_o):
        assert a <= 2 * b, line
    with _env("PDN_NORM_PLANES", "0"):
        off = P.entry(beta)
    assert _launches(P.L) - n0 == 2                          # (the switched-off call counted nothing)
    assert np.array_equal(_bits(off), _bits(old)), "switch off differs from the existing route"


def test_a_nan_row_marks_the_same_entries(hip):
    P = _problem(SHAPES[0])
    x = P.x.copy()
    x[12345] = np.nan
    xd = P.hp.from_numpy(x)
    xn, rms = P.forward(xd)
    new, old = P.entry(0.0, xd, rms), P.existing(0.0, xn)
    assert np.isnan(old).any() and np.array_equal(np.isnan(new), np.isnan(old))
    print(f"NaN row: {int(np.isnan(new).sum())} of {new.size} entries NaN in both")


# ---- node level -----------------------------------------------------------------------------------------------------------
def test_backward_with_the_switch_on_and_off(hip):
    from pydynet_amd.core import fused
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    L, hp = _lib_hp()
    _CACHE.clear()
    B, Lq = 256, 256                                         # 65536 tokens
    rng = np.random.default_rng(3)
    ids, tgt = rng.integers(0, 512, (B, Lq)), rng.integers(0, 512, (B, Lq))
    emb = (0.02 * rng.standard_normal((512, 288))).astype(np.float32)

    def step(on):
        old = fused.ffn_swiglu.norm_planes, fused.qkv_attention.norm_planes
        fused.ffn_swiglu.norm_planes = fused.qkv_attention.norm_planes = on
        try:
            np.random.seed(0)
            model = Llama(512, 288, 6, 768, Lq, B, 2, np.float32)
            model.tok_embedding.weight.data[...] = emb
            model.to("hip:0")
            Adam(model.parameters(), lr=0.0).flatten_grads()   # equally spaced gradients: the stacked products
            n0 = _launches(L)
            loss = model.loss(ids, tgt)
            loss.backward()
            grads = {n: q.grad.get() for n, q in model.named_parameters()}
            return float(loss.numpy()), grads, _launches(L) - n0
        finally:
            fused.ffn_swiglu.norm_planes, fused.qkv_attention.norm_planes = old

    l1, g1, n1 = step(True)
    l0, g0, n0 = step(False)
    assert n1 == 4 and n0 == 0, (n1, n0)                     # two per layer
    assert abs(l1 - l0) <= 1e-4 * abs(l0)
    worst = 0.0
    for name in g0:
        err = float(np.abs(g1[name] - g0[name]).max()) / max(float(np.abs(g0[name]).max()), 1e-12)
        worst = max(worst, err)
        assert err <= 1e-4, (name, err)
    print(f"node level, 65536 tokens: plane launches {n1}, loss {l1:.6f} / {l0:.6f}, worst gradient difference {worst:.2e}")
