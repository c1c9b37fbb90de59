"""NumPy emulation of the plane pass that forms an RMSNorm output on the way into the fp16 planes (stn_split_xn_kernel of
csrc/split_tn_planes.hip), beside tests/test_outres_tn_split_cpu.py whose pieces it uses:

    xn[t][d] = x[t][d] * (1 / r[t]) * w[d]   in fp32, r[t] = sqrt(mean_d x[t][d]^2 + eps) in fp32
    xn[:, d] 2^s(d) = xh + xl / 2048         s(d) = ls_shift(17 |w[d]|): the exponent of the BOUND |xn[t][d]| < 17 |w[d]|
                                             (|x[t][d]| <= sqrt(288) r[t]), not of the column's largest magnitude

32768 tokens x 288 of rows chosen to stress the bound, shuffled: standard normal; one-hot (|x_d| / r reaches sqrt(288); only in
the first 144 columns, so that the others' largest magnitude stays a few units and their exponent really moves); rows scaled by
1e30 (their squares overflow: r = Inf, xn = 0) and by 1e-30 (their squares vanish: r = sqrt(eps)); column 150 always 1e-4 of
its row's r.  Norm weights by column class: ordinary (0.5 .. 1.5), negative, 1e-20, 1e20, zero.

Asserted: |xn 2^s| < 2^9 (1 + 2^-20) for every element, no plane of these finite inputs is non-finite; and with the
three-product dW against float64 (the emulation of tests/test_outres_tn_split_cpu.py), the worst figure of every column class
with the bound's exponents <= 2 x that with the exact column maxima -- the project's standing criterion, here for the
emulation alone.  Figure of dW row d: largest |error| over the columns of g, divided by max_t |xn[t][d]| max |g|.  Both
figures are printed.

fp16 subnormals: the kernels run in the compiler's default mode, which keeps them, and that is the emulation every class is
held to.  The emulation with subnormal planes FLUSHED runs as well and holds every class to the same 2 x but one: the column
that is CONSTANT at 1e-4 of its row's r lies 2^-17 under the bound, its l plane is 2^-10 at most, and the one value all its
rows share happens to split into an l below 2^-14 -- flushed, the same 2^-25 is lost in every token instead of in one of
sixteen.  Measured there: 1.04e-4 with the bound's exponents against 4.03e-5 with the exact maximum (2.6 x); printed, not
asserted, and only a machine that flushed fp16 subnormals in its MFMA inputs would see it.  With the exact maxima the same
column sits at the top of its own range, which is what the three launches bought."""
import numpy as np
import pytest

from tests.test_outres_tn_split_cpu import D, S_UNSET, _planes, next_scale, x_shifts

K, V, EPS = 32768, 48, np.float32(1e-6)
CLASSES = {"ordinary": slice(0, 288), "negative": slice(20, 40), "1e-20": slice(160, 170), "1e20": slice(170, 180),
           "zero": slice(180, 184), "tiny column": slice(150, 151)}


def bound_shifts(w):
    """ls_shift(17 |w[d]|) in fp32: 0 for a zero or non-finite bound"""
    with np.errstate(over="ignore"):
        b = (np.float32(17.0) * np.abs(w)).astype(np.float32)
    _, E = np.frexp(b)
    return np.where(np.isfinite(b) & (b > 0), 9 - E, 0).astype(np.int32)


def emulate(xn, sh, g, flush):
    """dW (288, V) from planes of xn at the exponents sh, as emulate_split of tests/test_outres_tn_split_cpu.py in one K range"""
    xh, xl = _planes(np.ldexp(xn, sh[None, :]).astype(np.float32), flush)
    G = V // 16
    S = np.full(G, S_UNSET, np.int64)
    acc0, acc1 = np.zeros((D, V), np.float32), np.zeros((D, V), np.float32)
    for t0 in range(0, K, 32):
        gp = g[t0:t0 + 32]
        bits = gp.view(np.uint32) & np.uint32(0x7fffffff)
        Sn = next_scale(bits.reshape(32, G, 16).max((0, 2)), S)
        assert np.all((Sn == S) | (S == S_UNSET))           # g is flat: the running exponent is set once
        S = Sn
        gh, gl = _planes(np.ldexp(gp, np.repeat(S, 16)[None, :].astype(np.int32)).astype(np.float32), flush)
        a, b = xh[t0:t0 + 32].T, xl[t0:t0 + 32].T
        acc0 = (acc0 + a @ gh).astype(np.float32)
        acc1 = (acc1 + (b @ gh + a @ gl)).astype(np.float32)
    Se = np.repeat(S, 16)[None, :]
    return np.ldexp((acc0 + acc1 * np.float32(1.0 / 2048.0)).astype(np.float32), (-(Se + sh[:, None])).astype(np.int32))


def make_problem():
    rng = np.random.default_rng(17)
    x = rng.standard_normal((K, D), dtype=np.float32)
    kind = rng.permutation(np.repeat(np.arange(4), [K // 2, K // 4, K // 8, K // 8]))
    hot = np.flatnonzero(kind == 1)
    x[hot] = 0.0
    x[hot, rng.integers(0, 144, hot.size)] = (rng.choice([-1.0, 1.0], hot.size) * 10.0 ** rng.uniform(-3, 3, hot.size)).astype(np.float32)
    x[kind == 2] *= np.float32(1e30)
    x[kind == 3] *= np.float32(1e-30)
    w = rng.uniform(0.5, 1.5, D).astype(np.float32)
    w[CLASSES["negative"]] *= -1
    w[CLASSES["1e-20"]] *= np.float32(1e-20)
    w[CLASSES["1e20"]] *= np.float32(1e20)
    w[CLASSES["zero"]] = 0.0

    def rms_of(x):
        with np.errstate(over="ignore"):
            return np.sqrt((x * x).sum(-1, dtype=np.float32) / np.float32(288.0) + EPS).astype(np.float32)
    r = rms_of(x)
    x[:, 150] = np.where(np.isfinite(r), np.float32(1e-4) * r, np.float32(1e-4) * np.abs(x).max(-1))
    r = rms_of(x)
    with np.errstate(over="ignore", under="ignore"):
        inv = (np.float32(1.0) / r).astype(np.float32)
        xn = ((x * inv[:, None]).astype(np.float32) * w[None, :]).astype(np.float32)
    g = rng.standard_normal((K, V), dtype=np.float32)
    return x, w, r, xn, g


@pytest.fixture(scope="module")
def problem():
    return make_problem()


def test_every_element_is_below_the_bound_and_every_plane_finite(problem):
    x, w, r, xn, g = problem
    assert np.isfinite(x).all() and np.isfinite(w).all() and np.isfinite(xn).all()
    assert np.isinf(r).any() and (r == np.sqrt(EPS)).any()                  # both extreme row scales are present
    hot = np.abs(xn[:, :144] / np.where(w[:144] == 0, 1, w[:144])).max()
    assert 16.9 < hot < 17.0                                               # a one-hot row reaches sqrt(288)
    sh = bound_shifts(w)
    assert np.all(sh[CLASSES["zero"]] == 0)
    scaled = np.ldexp(xn.astype(np.float64), sh[None, :])
    assert np.abs(scaled).max() < 2.0 ** 9 * (1 + 2.0 ** -20)
    nz = w != 0
    assert np.abs(scaled[:, nz]).max(0).min() > 0                           # (every such column holds something)
    for flush in (False, True):
        h, l = _planes(np.ldexp(xn, sh[None, :]).astype(np.float32), flush)
        assert np.isfinite(h).all() and np.isfinite(l).all()
    # where the exact maxima give another exponent, it is the larger one: the bound never exceeds what the maximum allows
    ex = x_shifts(xn)
    assert np.all(ex[nz] >= sh[nz]) and np.any(ex[nz] > sh[nz])
    print(f"exponents: bound below the exact maximum's by {np.bincount((ex - sh)[nz]).tolist()} places (count per 0, 1, 2, ..)")


@pytest.mark.parametrize("flush", [False, True], ids=["kept", "flushed"])
def test_bound_exponents_within_twice_the_exact_maxima(problem, flush):
    x, w, r, xn, g = problem
    ref = xn.astype(np.float64).T @ g.astype(np.float64)
    amax, gmax = np.abs(xn).max(0).astype(np.float64), float(np.abs(g).max())
    figs = {}
    for name, sh in (("bound", bound_shifts(w)), ("exact", x_shifts(xn))):
        got = emulate(xn, sh, g, flush)
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - ref).max(1)
        assert not err[amax == 0].any()                      # a zero norm weight: the row of dW is exactly zero
        figs[name] = np.where(amax > 0, err / np.where(amax > 0, amax * gmax, 1.0), 0.0)
    for cname, sl in CLASSES.items():
        b, e = float(figs["bound"][sl].max()), float(figs["exact"][sl].max())
        print(f"{'flushed' if flush else 'kept':8s} {cname:12s} bound {b:.3e}  exact maxima {e:.3e}")
        if not (flush and cname in ("ordinary", "tiny column")):
            assert b <= 2 * e, (cname, b, e)
    if flush:                                                # every column but the constant one, and that one finite
        rest = np.ones(D, bool)
        rest[CLASSES["tiny column"]] = False
        b, e = float(figs["bound"][rest].max()), float(figs["exact"][rest].max())
        print(f"flushed  all but the constant column: bound {b:.3e}  exact maxima {e:.3e}")
        assert b <= 2 * e, (b, e)
