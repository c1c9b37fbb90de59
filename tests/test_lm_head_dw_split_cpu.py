"""The arithmetic of the split-fp16 lm_head weight gradient (csrc/lm_head_dw_split.hip) in NumPy, against float64.

    dW[d][v] = sum_t x[t][d] g[t][v],   g = exp(logit - lse[t]) - [v == target[t]]        (|g| <= 1)

The kernel forms g in fp32 from the fp32 logits, the one-hot included, scales it by 2^15 and splits it into two fp16 planes,
g 2^15 = gh + gl / 2048; every column d of x (a row of dW) gets its own power of two (largest magnitude over ALL tokens into
[2^8, 2^9)) and the same split; dW 2^(15 + s(d)) = xh gh + (xh gl + xl gh) / 2048 -- fp16 products are exact in fp32, the
sums are fp32 -- and the scales leave in one ldexp.  `_shift` / `_planes` are those of the forward's test.

The contraction runs over the TOKENS, tens of thousands of them, and what limits the accuracy of either kernel is the length
of its fp32 running sums: the kernels cut the tokens into K ranges whose partial sums are added afterwards.  The emulation
follows the matrix pipe piece by piece: every 32-token piece is a float64 dot product rounded to fp32 and added to an fp32
accumulator, one accumulator set per K range, the ranges added in fp32 at the end.

Inputs: default_rng(21), 32768 tokens, x ~ N(0, 1) (32768 x 288) with x[:, 17] *= 1e-6, w ~ 0.05 N(0, 1) (288 x 1024),
b ~ 0.1 N(0, 1), every 7th token targets column 5 (the "hot" column: its g is -1 + p there, the largest entries of g).
Figure: max_v |err| / max_t |x[t, d]| per row d of dW, then the max over d; over the ordinary columns, over row d = 17 alone
(the 1e-6 column of x) and over the hot column alone.

What is asserted, at 1, 2 and 8 K ranges: three fp16 products, subnormals kept AND flushed, are within 2 x the figure of the
same emulation fed the fp32 operands, AT THE SAME NUMBER OF RANGES, for each of the three figures; three bf16 products are
not (ordinary columns).

Dependence on the range count, measured here (fp32 operands | fp16 x 3, ordinary columns; hot column):
    1 range   8.16e-06 | 8.83e-06;   4.14e-05 | 5.32e-05
    2 ranges  5.16e-06 | 4.99e-06;   3.12e-05 | 2.85e-05
    8 ranges  1.85e-06 | 1.91e-06;   1.18e-05 | 1.28e-05
(row 17, the 1e-6 column of x: 4.36e-06 | 4.92e-06, 2.12e-06 | 2.86e-06, 1.11e-06 | 1.39e-06; flushing the fp16 subnormals
changes none of these digits; bf16 x 3: 2.5e-05 at every range count)
Each halving of the range count roughly doubles both: a split kernel that cut K into FEWER ranges than the fp32 kernel does
for the same shape would lose a comparison against it through summation length alone, which is why the kernel takes the
fp32 kernel's ranges (pdn_gemm_outres_tn_plan)."""
import numpy as np
import pytest

from tests.test_lm_head_split_cpu import _planes, _shift

K, V, T = 288, 1024, 32768
S_G = 15                                                 # LDW_ES of csrc/lm_head_dw_split.hip
HOT, D_TINY = 5, 17
RANGES = (1, 2, 8)
NP = T // 32


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(21)
    x = rng.standard_normal((T, K), dtype=np.float32)
    x[:, D_TINY] *= np.float32(1e-6)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    t = rng.integers(0, V, T)
    t[::7] = HOT
    logits = (x @ w + b).astype(np.float32)
    l64 = logits.astype(np.float64)
    m = l64.max(1)
    lse = (m + np.log(np.exp(l64 - m[:, None]).sum(1))).astype(np.float32)
    # g as the kernels form it, in fp32: one fma, one exp2, one select-subtract
    g = np.exp2(logits * np.float32(1.4426950408889634) - lse[:, None] * np.float32(1.4426950408889634)).astype(np.float32)
    g[np.arange(T), t] -= np.float32(1.0)
    ref = x.astype(np.float64).T @ g.astype(np.float64)  # exact for the g the kernels see
    return dict(x=x, g=g, ref=ref, xmax=np.abs(x.astype(np.float64)).max(0))


def _piecewise(terms):
    """terms: list of (A (T x K), B (T x V)) float32 pairs whose per-piece float64 products, each rounded to fp32, are added
    in turn to ONE fp32 accumulator per K range; returns {ranges: sum of the range accumulators, in fp32}"""
    acc = {r: np.zeros((r, K, V), np.float32) for r in RANGES}
    CH = 16
    t64 = [(np.ascontiguousarray(a.astype(np.float64).reshape(NP, 32, K).transpose(0, 2, 1)), bm.astype(np.float64).reshape(NP, 32, V))
           for a, bm in terms]
    buf64 = np.empty((CH, K, V), np.float64)
    dots = [np.empty((CH, K, V), np.float32) for _ in terms]
    for c0 in range(0, NP, CH):
        for (a3, b3), dt in zip(t64, dots):
            np.matmul(a3[c0:c0 + CH], b3[c0:c0 + CH], out=buf64)
            dt[...] = buf64
        for i in range(CH):
            p = c0 + i
            for r in RANGES:
                tgt = acc[r][p * r // NP]
                for dt in dots:
                    tgt += dt[i]
    out = {}
    for r in RANGES:
        s = acc[r][0].copy()
        for j in range(1, r):
            s += acc[r][j]
        out[r] = s
    return out


def _fp32_operands(d):
    return _piecewise([(d["x"], d["g"])])


def _split(d, fmt, ftz):
    sx = _shift(np.abs(d["x"]).max(0))
    xh, xl, up = _planes(d["x"], sx[None, :], fmt, ftz)
    gh, gl, _ = _planes(d["g"], np.int32(S_G), fmt, ftz)
    a0 = _piecewise([(xh, gh)])
    a1 = _piecewise([(xl, gh), (xh, gl)])                # the kernel's order: xl gh, then xh gl, into the same accumulator
    return {r: np.ldexp(a0[r] + a1[r] / up, -(S_G + sx[:, None])).astype(np.float32) for r in RANGES}


def _figures(dw, d):
    err = np.abs(dw.astype(np.float64) - d["ref"]) / d["xmax"][:, None]
    ordinary = np.delete(err, HOT, axis=1)
    return float(ordinary.max()), float(ordinary[D_TINY].max()), float(err[:, HOT].max())


@pytest.fixture(scope="module")
def fp32_figures(data):
    dw = _fp32_operands(data)
    return {r: _figures(dw[r], data) for r in RANGES}


@pytest.mark.parametrize("ftz", [False, True])
def test_three_fp16_products_match_fp32_operands_at_equal_ranges(data, fp32_figures, ftz):
    dw = _split(data, "fp16", ftz)
    for r in RANGES:
        s, f = _figures(dw[r], data), fp32_figures[r]
        print(f"{r} K ranges, ftz={ftz}: ordinary columns fp16 x 3 {s[0]:.3e} (fp32 operands {f[0]:.3e}); row {D_TINY} "
              f"{s[1]:.3e} ({f[1]:.3e}); hot column {s[2]:.3e} ({f[2]:.3e})")
        assert s[0] <= 2.0 * f[0], ("ordinary", r, s[0], f[0])
        assert s[1] <= 2.0 * f[1], ("the 1e-6 column of x", r, s[1], f[1])
        assert s[2] <= 2.0 * f[2], ("hot column", r, s[2], f[2])


def test_three_bf16_products_do_not(data, fp32_figures):
    dw = _split(data, "bf16", False)
    for r in RANGES:
        s, f = _figures(dw[r], data), fp32_figures[r]
        print(f"{r} K ranges: ordinary columns bf16 x 3 {s[0]:.3e} (fp32 operands {f[0]:.3e})")
        assert not s[0] <= 2.0 * f[0], (r, s[0], f[0])


def test_fewer_ranges_cost_accuracy(fp32_figures):
    """the reason for the kernel's K-range rule: the fp32 figure itself grows as the ranges get longer"""
    assert fp32_figures[1][0] > 1.5 * fp32_figures[8][0] and fp32_figures[1][2] > 1.5 * fp32_figures[8][2]


def test_planes_stay_inside_fp16(data):
    gh, gl, _ = _planes(data["g"], np.int32(S_G), "fp16", False)
    assert np.isfinite(gh).all() and np.isfinite(gl).all()
    assert np.abs(gh).max() <= 2.0 ** S_G and np.abs(gl).max() <= 2.0 ** 15
    sx = _shift(np.abs(data["x"]).max(0))
    xh, xl, _ = _planes(data["x"], sx[None, :], "fp16", False)
    assert np.isfinite(xh).all() and np.isfinite(xl).all() and np.abs(xh).max() < 2.0 ** 9
