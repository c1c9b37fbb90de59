"""The gradient-clipping kernels of csrc/optim.hip through the raw C ABI (as test_adam_multi_matches_reference_update does for
Adam): the multi-tensor norm, its coefficient and control words, the Adam update that consumes them (L2 and decoupled decay),
the skipped step on a non-finite norm, and the stand-alone gradient scale."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CH = 16384
NORM_SIZES = [1, 7, CH, CH + 3, 5 * CH]          # below a vector, one chunk exactly, a boundary with a 3-element tail, several
ADAM_SIZES = [288 * 288, 288, 1000, 7]
ULP2 = 2.5e-7                                    # two float32 ulps: the device sums exact squares in double, so only the
#                                                  final rounding to float32 separates it from the float64 reference


def chunk_rows(arrays):
    """Adam's chunk table over (p, g, m, v) device arrays per tensor; absent columns are 0 (the norm reads g and n only)."""
    rows = []
    for p, g, m, v in arrays:
        for off in range(0, g.size, CH):
            rows.append([a._ptr + 4 * off if a is not None else 0 for a in (p, g, m, v)] + [min(CH, g.size - off)])
    return np.asarray(rows, dtype=np.int64)


class Norm:
    """Gradients of NORM_SIZES on the device (the second starts one element into its buffer: 4-byte aligned only, the scalar
    loads run), their table, partials and control words, and the float64 reference norm -- built once for the module."""

    def __init__(self, hip):
        rng = np.random.default_rng(31)
        self.G = [rng.standard_normal(n, dtype=np.float32) for n in NORM_SIZES]
        self.dG = [hip.from_numpy(g) for g in self.G]
        shifted = hip.from_numpy(np.concatenate([np.zeros(1, np.float32), self.G[3]]))
        self.dG[3] = shifted[1:]
        assert self.dG[3]._ptr % 16 == 4 and self.dG[4]._ptr % 16 == 0
        rows = chunk_rows([(None, g, None, None) for g in self.dG])
        self.n = len(rows)
        self.table = hip.from_numpy(rows)
        self.partials = hip.zeros((self.n,), np.float64)
        self.ctl = hip.zeros((4,), np.float32)
        self.ref = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in self.G))

    def measure(self, hip, L, grad_scale, max_norm):
        L.call("pdnx_grad_norm_multi_f32", self.table._ptr, self.n, grad_scale, max_norm, self.partials._ptr, self.ctl._ptr,
               hip.stream())
        return self.ctl.get(), self.partials.get()


@pytest.fixture(scope="module")
def norm(hip):
    return Norm(hip)


def rel(a, b):
    return abs(float(a) - b) / abs(b)


def test_norm_matches_float64_and_repeats_bit_for_bit(hip, norm):
    from pydynet_amd import _lib
    L = _lib.lib()
    assert norm.n == 1 + 1 + 1 + 2 + 5
    for scale in (1.0, 0.5):
        ctl, part = norm.measure(hip, L, scale, 0.0)
        print("norm", scale, ctl[0], norm.ref * scale, rel(ctl[0], norm.ref * scale))
        assert rel(ctl[0], norm.ref * scale) <= ULP2
        assert ctl[1] == 1.0 and ctl[2] == 0.0                      # max_norm 0: measure only
        ctl2, part2 = norm.measure(hip, L, scale, 0.0)
        assert ctl2[0].tobytes() == ctl[0].tobytes() and part2.tobytes() == part.tobytes()
    ref_parts = np.concatenate([[float((g[o:o + CH].astype(np.float64) ** 2).sum()) for o in range(0, g.size, CH)]
                                for g in norm.G])
    # a chunk's partial: at most 2^14 exact squares, added in another order than NumPy's (under a hundred roundings at 2^-53 each)
    assert np.allclose(part, ref_parts, rtol=1e-13, atol=0)


def test_coefficient(hip, norm):
    from pydynet_amd import _lib
    L = _lib.lib()
    ctl, _ = norm.measure(hip, L, 1.0, 2 * norm.ref)
    assert ctl[1] == 1.0 and ctl[2] == 0.0
    max_norm = norm.ref / 4
    ctl, _ = norm.measure(hip, L, 1.0, max_norm)
    print("coef", ctl[1], max_norm / (norm.ref + 1e-6), rel(ctl[1], max_norm / (norm.ref + 1e-6)))
    assert rel(ctl[1], max_norm / (norm.ref + 1e-6)) <= ULP2 and ctl[2] == 0.0
    ctl, _ = norm.measure(hip, L, 1.0, 0.0)
    assert ctl[1] == 1.0


def test_scale_multiplies_by_the_coefficient_exactly(hip, norm):
    from pydynet_amd import _lib
    L = _lib.lib()
    ctl, _ = norm.measure(hip, L, 1.0, norm.ref / 4)
    try:
        L.call("pdnx_grad_scale_multi_f32", norm.table._ptr, norm.n, norm.ctl._ptr, hip.stream())
        for d, g in zip(norm.dG, norm.G):
            assert np.array_equal(d.get(), g * np.float32(ctl[1]))
        # skip set: untouched
        norm.ctl[...] = hip.from_numpy(np.array([ctl[0], 0.0, 1.0, 0.0], np.float32))
        before = [d.get() for d in norm.dG]
        L.call("pdnx_grad_scale_multi_f32", norm.table._ptr, norm.n, norm.ctl._ptr, hip.stream())
        for d, b in zip(norm.dG, before):
            assert np.array_equal(d.get(), b)
    finally:                                                        # the module's gradients and ctl as the other tests expect them
        for d, g in zip(norm.dG, norm.G):
            d[...] = hip.from_numpy(g)
        norm.ctl[...] = hip.zeros((4,), np.float32)


def adam_state(hip, seed=12):
    rng = np.random.default_rng(seed)
    P = [rng.standard_normal(n, dtype=np.float32) for n in ADAM_SIZES]
    G = [rng.standard_normal(n, dtype=np.float32) for n in ADAM_SIZES]
    M = [np.zeros(n, np.float32) for n in ADAM_SIZES]
    V = [np.zeros(n, np.float32) for n in ADAM_SIZES]
    dev = [[hip.from_numpy(a) for a in lst] for lst in (P, G, M, V)]
    rows = chunk_rows(list(zip(*dev)))
    return (P, G, M, V), dev, hip.from_numpy(rows), len(rows)


@pytest.mark.parametrize("decoupled,clip", [(0, True), (1, True), (1, False)], ids=["l2-clip", "decoupled-clip", "adamw-noclip"])
def test_update_matches_the_float64_statement(hip, decoupled, clip):
    """Three steps of norm + update, every one clipping (max_norm = norm / 4), against optim/clip.py's statement in float64
    cast per step; tolerances of test_adam_multi_matches_reference_update."""
    from pydynet_amd import _lib
    L = _lib.lib()
    (P, G, M, V), (dP, dG, dM, dV), table, n = adam_state(hip)
    partials, ctl = hip.zeros((n,), np.float64), hip.zeros((4,), np.float32)
    lr, b1, b2, eps, wd, gs = 1e-3, 0.9, 0.999, 1e-8, 0.01, 0.5
    norm = gs * math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in G))
    max_norm = norm / 4
    coef = min(1.0, max_norm / (norm + 1e-6)) if clip else 1.0
    assert not clip or coef < 0.26
    for t in (1, 2, 3):
        a_t = math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        if clip:
            L.call("pdnx_grad_norm_multi_f32", table._ptr, n, gs, max_norm, partials._ptr, ctl._ptr, hip.stream())
        L.call("pdnx_adam_multi_clip_f32", table._ptr, n, lr * a_t, lr * wd, b1, b2, eps, wd, gs, decoupled,
               ctl._ptr if clip else None, hip.stream())
        for i in range(len(ADAM_SIZES)):
            p, g, m, v = (a[i].astype(np.float64) for a in (P, G, M, V))
            gg = g * gs * coef
            if decoupled:
                p = p - lr * wd * p
            else:
                gg = gg + wd * p
            m = b1 * m + (1 - b1) * gg
            v = b2 * v + (1 - b2) * gg ** 2
            p = p - lr * a_t * m / (np.sqrt(v) + eps)
            P[i], M[i], V[i] = p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)
    if clip:
        assert ctl.get()[2] == 0.0 and rel(ctl.get()[1], coef) <= ULP2
    for i in range(len(ADAM_SIZES)):
        assert np.allclose(dP[i].get(), P[i], rtol=1e-5, atol=1e-7)
        assert np.allclose(dM[i].get(), M[i], rtol=1e-5, atol=1e-8)
        assert np.allclose(dV[i].get(), V[i], rtol=1e-5, atol=1e-10)
        assert np.array_equal(dG[i].get(), G[i])                    # gradients in memory are not rewritten


@pytest.mark.parametrize("bad", [np.inf, np.nan], ids=["inf", "nan"])
def test_non_finite_norm_skips_the_update_and_counts(hip, bad):
    from pydynet_amd import _lib
    L = _lib.lib()
    (P, G, M, V), (dP, dG, dM, dV), table, n = adam_state(hip, seed=13)
    partials, ctl = hip.zeros((n,), np.float64), hip.zeros((4,), np.float32)

    def step(decoupled):
        L.call("pdnx_grad_norm_multi_f32", table._ptr, n, 1.0, 1.0, partials._ptr, ctl._ptr, hip.stream())
        L.call("pdnx_adam_multi_clip_f32", table._ptr, n, 1e-3, 1e-5, 0.9, 0.999, 1e-8, 0.01, 1.0, decoupled, ctl._ptr,
               hip.stream())
        return ctl.get()

    c = step(0)                                                     # a finite step first: m and v are not all zero
    assert c[2] == 0.0 and c[3] == 0.0 and 0.0 < c[1] < 1.0
    g = G[0].copy()
    g[20000] = bad                                                  # in the second chunk of the first tensor
    dG[0][...] = hip.from_numpy(g)
    before = [a.get() for a in dP + dM + dV]
    for count, decoupled in ((1, 0), (2, 1)):
        c = step(decoupled)
        assert c[2] == 1.0 and c[1] == 0.0 and c[3] == count, c
        assert all(x.tobytes() == a.get().tobytes() for x, a in zip(before, dP + dM + dV))
    ctl[...] = hip.zeros((4,), np.float32)                          # the caller's reset is respected
    assert step(0)[3] == 1.0
    dG[0][...] = hip.from_numpy(G[0])
    c = step(0)                                                     # finite again: the step runs, the count stays
    assert c[2] == 0.0 and c[3] == 1.0
    assert not np.array_equal(dP[0].get(), before[0])


def test_argument_checks(hip, norm):
    from pydynet_amd import _lib
    L = _lib.lib()
    st = hip.stream()
    L.call("pdnx_grad_norm_multi_f32", None, 0, 1.0, 1.0, None, None, st)               # nchunks == 0 is fine everywhere
    L.call("pdnx_grad_scale_multi_f32", None, 0, None, st)
    L.call("pdnx_adam_multi_clip_f32", None, 0, 1e-3, 0.0, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None, st)
    for name, args in (("pdnx_grad_norm_multi_f32", (norm.table._ptr, norm.n, 1.0, 1.0, norm.partials._ptr, None, st)),
                       ("pdnx_grad_norm_multi_f32", (None, norm.n, 1.0, 1.0, norm.partials._ptr, norm.ctl._ptr, st)),
                       ("pdnx_grad_scale_multi_f32", (norm.table._ptr, norm.n, None, st)),
                       ("pdnx_adam_multi_clip_f32", (None, 3, 1e-3, 0.0, 0.9, 0.999, 1e-8, 0.0, 1.0, 0, None, st)),
                       ("pdnx_adam_multi_clip_tick_f32", (norm.table._ptr, norm.n, None, None, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0,
                                                         0, norm.partials._ptr, norm.ctl._ptr, st))):
        with pytest.raises(_lib.HipLibraryError) as e:
            L.call(name, *args)
        assert e.value.code == -1
