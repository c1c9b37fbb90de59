"""NumPy emulation of the arithmetic of the split-fp16 output-resident products (csrc/outres_split.hip):

    C[t][d] = sum_k A[t][k] W[d][k]

    W[d, :] 2^s(d) = wh + wl / 2048        one power of two per output column d, the largest |W[d, :]| into [2^8, 2^9)
    A[t, :] 2^S(t) = ah + al / 2048        S(t): the RUNNING exponent of ROW t (ors_next_exp of csrc/outres_split_index.h),
                                           found piece by piece, no pass over A
    C 2^(S(t) + s(d)) = ah wh + (ah wl + al wh) / 2048        two fp32 running sums over pieces of 32 contraction values

Before the 32 values of a row's piece are split, their largest finite magnitude is taken; if that times 2^S would reach
2^15, or S is not set, S becomes the exponent that puts it into [2^12, 2^13), and both running sums of the row are multiplied
by the exact power of two between the old and the new S once the current piece is in.  S only falls; all-zero pieces are
ignored.

The emulation forms every piece's dot products in float64 from the fp16 planes (an MFMA's products of fp16 values are exact
in fp32 and its 32-term sum is not the error under study) and keeps the running sums in fp32.  The yardstick is an fp32
product summed in the same pieces of 32: fp32 operands, the piece's product formed in fp32 (NumPy's float32 matmul) and
added to an fp32 running sum -- what a pipe that multiplies and accumulates in fp32 does.  Everything runs twice: fp16
subnormal planes kept, and flushed to zero.

Figure: max_d |err[t][d]| / (max_k |A[t][k]| * max_k |W[d][k]|) against float64, the worst of 64 rows (a zero scale wants an
exact zero).  Row-scale kinds: flat; rows log-uniform over 1e-6 .. 1e3 (adjacent rows differ); rising and falling ramps
1e-8 .. 1e3 along k; 1e-30; one element 1e6 above its row near the end; an all-zero row; a row whose first half is zero.
Every W carries one row at 1e-6 of the others.  K over {768, 864, 1536}.

Bound: split <= 2 x the fp32 operands' figure (the rule of tests/test_outres_tn_split_cpu.py: the 2 allows for the rounding
points being different ones).  With the late outlier everything before it sits twenty octaves below the scale the row ends
at; there the kept form must be within 2 x of the flushed one's figure (twice the flushed figure on its own inputs is the
bound tests/test_outres_split_gpu.py uses for that kind).  The moves of S after it was first set are asserted too: none,
except one for the late outlier and, on the rising ramp, one per 2 .. 4.6 octaves (a move needs the maximum to climb from
below 2^13 to 2^15, and overshoots by at most three octaves less a bit plus a piece's growth of 1.6): 36.5 octaves and the
noise on top make 7 .. 20.

Figures of this file (kept and flushed agree to three digits but for one case, 6.49e-7 / 6.80e-7): split 0.5 .. 1.6 x the
fp32 product's on every kind but the late outlier (the 1.5 .. 1.6 at K = 1536, 1e-30 and half-zero rows), 1.25 .. 1.47 x
there; 8 .. 12 moves per row on the rising ramp, one on the outlier, none elsewhere; zero rows exactly zero."""
import numpy as np
import pytest

from tests.test_outres_tn_split_cpu import _planes

D = 288
S_UNSET = 1 << 20
KINDS = ["flat", "loguniform", "rising", "falling", "tiny", "outlier", "zero_row", "half_zero"]
KS = [768, 864, 1536]
ROWS = 64


def next_exp(mx, S):
    """ors_next_exp, vectorised over rows: mx float32 (largest finite magnitude, 0 = none), S int64"""
    _, E = np.frexp(mx)
    move = (mx > 0) & (E + S >= 16)
    return np.where(move, 13 - E, S)


def w_shifts(w):
    """ls_shift per output column (a row of w as stored): 0 for zero / non-finite"""
    amax = np.abs(w).max(1)
    _, E = np.frexp(amax)
    ok = np.isfinite(amax) & (amax > 0)
    return np.where(ok, 9 - E, 0).astype(np.int32)


def emulate_split(a, w, flush):
    """(T, K) x (288, K) float32 -> (C (T, 288) float32, moves of S per row after the first set)"""
    T, K = a.shape
    assert K % 32 == 0 and w.shape == (D, K)
    sh = w_shifts(w)
    wh, wl = _planes(np.ldexp(w, sh[:, None]).astype(np.float32), flush)
    S = np.full(T, S_UNSET, np.int64)
    acc0, acc1, moves = np.zeros((T, D), np.float32), np.zeros((T, D), np.float32), np.zeros(T, np.int64)
    for k0 in range(0, K, 32):
        ap = a[:, k0:k0 + 32]
        mag = np.abs(ap)
        mx = np.where(np.isfinite(mag), mag, np.float32(0)).max(1)
        Sn = next_exp(mx, S)
        with np.errstate(over="ignore", invalid="ignore"):
            ah, al = _planes(np.ldexp(ap, np.where(Sn == S_UNSET, 0, Sn)[:, None].astype(np.int32)).astype(np.float32), flush)
        moved = (Sn != S) & (S != S_UNSET)
        if moved.any():
            f = np.where(moved, Sn - S, 0)[:, None].astype(np.int32)
            acc0, acc1 = np.ldexp(acc0, f).astype(np.float32), np.ldexp(acc1, f).astype(np.float32)
            moves += moved
        S = Sn
        bh, bl = wh[:, k0:k0 + 32].T, wl[:, k0:k0 + 32].T
        with np.errstate(invalid="ignore"):
            acc0 = (acc0 + ah @ bh).astype(np.float32)
            acc1 = (acc1 + (ah @ bl + al @ bh)).astype(np.float32)
    Se = np.where(S == S_UNSET, 0, S)[:, None]
    with np.errstate(invalid="ignore"):
        out = np.ldexp((acc0 + acc1 * np.float32(1.0 / 2048.0)).astype(np.float32), (-(Se + sh[None, :])).astype(np.int32))
    return out.astype(np.float32), moves


def emulate_fp32(a, w):
    """an fp32 product summed in pieces of 32: fp32 operands, every piece's product formed and added in fp32"""
    acc = np.zeros((a.shape[0], D), np.float32)
    for k0 in range(0, a.shape[1], 32):
        acc = acc + a[:, k0:k0 + 32] @ w[:, k0:k0 + 32].T
    assert acc.dtype == np.float32
    return acc


def figure(got, a, w):
    """worst row of max_d |err| / (max_k |A[t]| max_k |W[d]|); where that scale is zero the result must be exactly zero"""
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    scale = np.abs(a).astype(np.float64).max(1)[:, None] * np.abs(w).astype(np.float64).max(1)[None, :]
    err = np.abs(got.astype(np.float64) - ref)
    assert (err[scale == 0] == 0).all()
    return float((err[scale > 0] / scale[scale > 0]).max())


def make_w(K, rng):
    w = rng.standard_normal((D, K), dtype=np.float32) * np.exp2(rng.integers(-3, 4, D)).astype(np.float32)[:, None]
    w[17] *= np.float32(1e-6)
    return w


def make_a(kind, T, K, rng):
    """T rows of the kind; "zero_row" / "half_zero" / "outlier" change rows of a flat matrix (every third, so that the
    sampled groups of the GPU test hold some)"""
    a = rng.standard_normal((T, K))
    if kind == "loguniform":
        a *= 10.0 ** rng.uniform(-6, 3, T)[:, None]
    elif kind == "rising":
        a *= 10.0 ** np.linspace(-8, 3, K)[None, :]
    elif kind == "falling":
        a *= 10.0 ** np.linspace(3, -8, K)[None, :]
    elif kind == "tiny":
        a *= 1e-30
    elif kind == "outlier":
        a[:, K - 40] *= 1e6
    elif kind == "zero_row":
        a[::3] = 0.0
    elif kind == "half_zero":
        a[::3, :K // 2] = 0.0
    else:
        assert kind == "flat"
    return a.astype(np.float32)


@pytest.fixture(scope="module")
def results():
    out = {}
    for K in KS:
        for i, kind in enumerate(KINDS):
            rng = np.random.default_rng(1000 * K + i)
            w, a = make_w(K, rng), make_a(kind, ROWS, K, rng)
            fp32 = figure(emulate_fp32(a, w), a, w)
            rec = {}
            for flush in (False, True):
                got, moves = emulate_split(a, w, flush)
                rec[flush] = (figure(got, a, w), fp32, moves, bool(np.isfinite(got).all()), got)
            out[K, kind] = rec
            print(f"K {K:4d} {kind:10s} fp32 {fp32:.3e}   split {rec[False][0]:.3e} / {rec[True][0]:.3e} (kept / flushed)"
                  f"   moves of S {int(rec[False][2].min())} .. {int(rec[False][2].max())}")
    return out


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "outlier"])
@pytest.mark.parametrize("K", KS)
def test_split_within_twice_the_fp32_operands(results, K, kind):
    for flush in (False, True):
        split, fp32, _, finite, got = results[K, kind][flush]
        assert finite and split <= 2.0 * fp32, (K, kind, flush, split, fp32)
        if kind == "zero_row":
            assert (got[::3] == 0).all()


@pytest.mark.parametrize("K", KS)
def test_late_outlier_is_finite_and_bounded(results, K):
    kept, flushed = results[K, "outlier"][False], results[K, "outlier"][True]
    assert kept[3] and flushed[3]
    assert kept[0] <= 2.0 * flushed[0], (kept[0], flushed[0])


@pytest.mark.parametrize("kind,lo,hi", [("flat", 0, 0), ("loguniform", 0, 0), ("rising", 7, 20), ("falling", 0, 0), ("tiny", 0, 0),
                                        ("outlier", 1, 1), ("zero_row", 0, 0), ("half_zero", 0, 0)])
@pytest.mark.parametrize("K", KS)
def test_moves_of_the_running_exponent(results, K, kind, lo, hi):
    for flush in (False, True):
        moves = results[K, kind][flush][2]
        assert lo <= moves.min() and moves.max() <= hi, (K, kind, moves)


def test_next_exp_rule():
    one = np.array([1.0], np.float32)
    assert next_exp(np.zeros(1, np.float32), np.array([S_UNSET]))[0] == S_UNSET           # an all-zero piece changes nothing
    assert next_exp(one, np.array([S_UNSET]))[0] == 12                                      # 1.0 2^12 in [2^12, 2^13)
    assert next_exp(one, np.array([14]))[0] == 14 and next_exp(one, np.array([15]))[0] == 12
    big = np.array([3.0e4], np.float32)                                                     # 2^14.87
    assert next_exp(big, np.array([0]))[0] == 0 and next_exp(big, np.array([1]))[0] == -2
