"""NumPy emulation of the arithmetic of the split-fp16 packed layer weight gradients (csrc/outres_tn_split.hip):

    dW[d][v] = sum_t x[t][d] g[t][v]

    x[:, d] 2^s(d) = xh + xl / 2048        one power of two per column d, the largest |x[:, d]| into [2^8, 2^9)
    g 2^S = gh + gl / 2048                 S: the RUNNING exponent of a wave's sixteen columns (ots_next_scale of
                                           csrc/split_tn_index.h), found piece by piece, no pass over g
    dW 2^(S + s(d)) = xh gh + (xh gl + xl gh) / 2048        two fp32 running sums over pieces of 32 tokens

Before the 32 x 16 values of a piece are split, their largest finite magnitude is taken; if that times 2^S would reach
2^15, S becomes the exponent that puts it into [2^12, 2^13) and both running sums are multiplied by the exact power of two
between the old and the new S once the current piece is in.  S starts from the first non-zero piece and only ever falls.

The emulation forms every piece's dot products in float64 from the fp16 planes (an MFMA's products of fp16 values are exact
in fp32 and its 32-term sum is not the error under study) and keeps the running sums in fp32, for the split form and for
fp32 operands alike.  It is not known whether the MFMA flushes fp16 subnormal inputs, so everything runs twice: subnormal
planes kept, and flushed to zero.  Figure: the largest |error| against float64 over the 288 x 48 outputs, divided by
max |x| * max_v max_t |g[t, v]|.

Six inputs, K = 8192 in one range: g's rows scaled flat, log-uniform over 1e-6 .. 1, on a geometric ramp 1e-8 -> 1e3 and
1e3 -> 1e-8, by 1e-30, and flat with ONE row scaled by 1e6.  On the first five the split form must be within 2 x of the fp32
operands' figure (the 2 allows for the rounding points being different ones; measured 1.0 .. 1.55 x with these inputs).  With
the single outlier row every other row sits twenty octaves below the scale S is set for; there the split form must be finite
and the kept form within 2 x of the flushed one's figure (twice that figure on its own inputs is the bound
tests/test_outres_tn_split_gpu.py uses for its outlier row).  In this emulation a flush of fp16 subnormals changes no
figure: a plane value below 2^-14 belongs to an operand 2^-22 of its column's or piece's largest, whose products are below
the fp32 rounding of the sums.  The number of times S moved after it
was first set is asserted too (0, 0, at least one on the rising ramp -- 36.5 octaves at one move per three --, 0, 0, 1), so
that the rescale path is known to run."""
import numpy as np
import pytest

D = 288
S_UNSET, S_TOP, S_AIM = 1 << 20, 15, 12
F16_MIN_NORMAL = 2.0 ** -14


def next_scale(mbits, S):
    """ots_next_scale, vectorised over the waves: mbits uint32 (largest finite magnitude as fp32 bits, 0 = none), S int."""
    E = (mbits >> 23).astype(np.int64)
    move = (mbits != 0) & (E - 127 + S >= S_TOP)
    return np.where(move, S_AIM + 127 - E, S)


def _f16(v, flush):
    with np.errstate(over="ignore", invalid="ignore"):
        h = v.astype(np.float16)
    if flush:
        h = np.where(np.abs(h) < F16_MIN_NORMAL, np.float16(0), h)
    return h


def _planes(vs, flush):
    """the two fp16 planes of fp32 values that are scaled already (ls_split_scaled), as float64"""
    h = _f16(vs, flush)
    with np.errstate(invalid="ignore"):
        l = _f16((vs - h.astype(np.float32)) * np.float32(2048.0), flush)
    return h.astype(np.float64), l.astype(np.float64)


def x_shifts(x):
    """ls_shift per column: the exponent that puts the column's largest magnitude into [2^8, 2^9); 0 for zero / non-finite"""
    amax = np.abs(x).max(0)
    _, E = np.frexp(amax)
    ok = np.isfinite(amax) & (amax > 0)
    return np.where(ok, 9 - E, 0).astype(np.int32)


def emulate_split(x, g, flush, kps=None):
    """(K, 288) x (K, V) float32, V a multiple of 16 -> (dW (288, V) float32, moves of S per wave after the first set, summed
    over the K ranges).  kps: tokens per K range (a multiple of 32); the ranges' results are added in fp32."""
    K, V = g.shape
    assert K % 32 == 0 and V % 16 == 0 and x.shape == (K, D)
    kps = K if kps is None else kps
    sh = x_shifts(x)
    xh, xl = _planes(np.ldexp(x, sh[None, :]).astype(np.float32), flush)
    G = V // 16
    total, moves = np.zeros((D, V), np.float32), np.zeros(G, np.int64)
    for k0 in range(0, K, kps):
        S = np.full(G, S_UNSET, np.int64)
        acc0, acc1 = np.zeros((D, V), np.float32), np.zeros((D, V), np.float32)
        for t0 in range(k0, min(K, k0 + kps), 32):
            gp = g[t0:t0 + 32]
            bits = gp.view(np.uint32) & np.uint32(0x7fffffff)
            bits = np.where(bits < np.uint32(0x7f800000), bits, np.uint32(0))
            Sn = next_scale(bits.reshape(32, G, 16).max((0, 2)), S)
            with np.errstate(over="ignore", invalid="ignore"):
                gs = np.ldexp(gp, np.repeat(np.where(Sn == S_UNSET, 0, Sn), 16)[None, :].astype(np.int32)).astype(np.float32)
            gh, gl = _planes(gs, flush)
            a, b = xh[t0:t0 + 32].T, xl[t0:t0 + 32].T
            # the planes of THIS piece were formed with Sn; the sums so far move to it first (on the GPU: after the piece
            # before this one, whose planes were formed with the old S)
            moved = (Sn != S) & (S != S_UNSET)
            if moved.any():
                f = np.repeat(np.where(moved, Sn - S, 0), 16)[None, :].astype(np.int32)
                acc0, acc1 = np.ldexp(acc0, f).astype(np.float32), np.ldexp(acc1, f).astype(np.float32)
                moves += moved
            S = Sn
            with np.errstate(invalid="ignore"):
                acc0 = (acc0 + a @ gh).astype(np.float32)
                acc1 = (acc1 + (b @ gh + a @ gl)).astype(np.float32)
        Se = np.repeat(np.where(S == S_UNSET, 0, S), 16)[None, :]
        with np.errstate(invalid="ignore"):
            part = np.ldexp((acc0 + acc1 * np.float32(1.0 / 2048.0)).astype(np.float32), (-(Se + sh[:, None])).astype(np.int32))
            total = (total + part.astype(np.float32)).astype(np.float32)
    return total, moves


def emulate_fp32(x, g, flush, kps=None):
    """the same running sums with fp32 operands (flush: fp32 subnormal operands read as zero)"""
    K, V = g.shape
    kps = K if kps is None else kps
    if flush:
        tiny = np.float32(2.0 ** -126)
        x, g = np.where(np.abs(x) < tiny, np.float32(0), x), np.where(np.abs(g) < tiny, np.float32(0), g)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    total = np.zeros((D, V), np.float32)
    for k0 in range(0, K, kps):
        acc = np.zeros((D, V), np.float32)
        for t0 in range(k0, min(K, k0 + kps), 32):
            acc = (acc + x64[t0:t0 + 32].T @ g64[t0:t0 + 32]).astype(np.float32)
        total = (total + acc).astype(np.float32)
    return total


def figure(got, x, g):
    ref = x.astype(np.float64).T @ g.astype(np.float64)
    return float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(x).max() * np.abs(g).max()))


K, V = 8192, 48


def _x(rng):
    return (rng.standard_normal((K, D), dtype=np.float32) * np.exp2(rng.integers(-6, 7, D)).astype(np.float32)[None, :])


def _rows(kind, rng):
    if kind == "flat":
        return np.ones(K)
    if kind == "loguniform":
        return 10.0 ** rng.uniform(-6, 0, K)
    if kind == "rising":
        return 10.0 ** np.linspace(-8, 3, K)
    if kind == "falling":
        return 10.0 ** np.linspace(3, -8, K)
    if kind == "tiny":
        return np.full(K, 1e-30)
    assert kind == "outlier"
    r = np.ones(K)
    r[K // 3] = 1e6
    return r


@pytest.fixture(scope="module")
def results():
    out = {}
    for i, kind in enumerate(("flat", "loguniform", "rising", "falling", "tiny", "outlier")):
        rng = np.random.default_rng(100 + i)
        x = _x(rng)
        g = (rng.standard_normal((K, V)) * _rows(kind, rng)[:, None]).astype(np.float32)
        rec = {}
        for flush in (False, True):
            got, moves = emulate_split(x, g, flush)
            rec[flush] = (figure(got, x, g), figure(emulate_fp32(x, g, flush), x, g), moves, bool(np.isfinite(got).all()))
        out[kind] = rec
        print(f"{kind:11s} fp32 {rec[False][1]:.3e} / {rec[True][1]:.3e}   split {rec[False][0]:.3e} / {rec[True][0]:.3e}"
              f"   (kept / flushed)   moves of S {rec[False][2].tolist()}")
    return out


@pytest.mark.parametrize("kind", ["flat", "loguniform", "rising", "falling", "tiny"])
def test_split_within_twice_the_fp32_operands(results, kind):
    for flush in (False, True):
        split, fp32, _, finite = results[kind][flush]
        assert finite and split <= 2.0 * fp32, (kind, flush, split, fp32)


def test_outlier_row_is_finite_and_bounded(results):
    (kept, _, _, fin_k), (flushed, _, _, fin_f) = results["outlier"][False], results["outlier"][True]
    assert fin_k and fin_f
    assert kept <= 2.0 * flushed, (kept, flushed)


@pytest.mark.parametrize("kind,want", [("flat", 0), ("loguniform", 0), ("rising", None), ("falling", 0), ("tiny", 0), ("outlier", 1)])
def test_moves_of_the_running_exponent(results, kind, want):
    for flush in (False, True):
        moves = results[kind][flush][2]
        if want is None:
            assert (moves >= 1).all(), moves
        else:
            assert (moves == want).all(), moves


def test_next_scale_rule():
    one = np.array([np.float32(1.0).view(np.uint32)], np.uint32)
    assert next_scale(np.zeros(1, np.uint32), np.array([S_UNSET]))[0] == S_UNSET         # an all-zero piece changes nothing
    assert next_scale(one, np.array([S_UNSET]))[0] == 12                                    # 1.0 2^12 in [2^12, 2^13)
    assert next_scale(one, np.array([14]))[0] == 14 and next_scale(one, np.array([15]))[0] == 12
    big = np.array([np.float32(3.0e4).view(np.uint32)], np.uint32)                          # 2^14.87
    assert next_scale(big, np.array([0]))[0] == 0 and next_scale(big, np.array([1]))[0] == -2
