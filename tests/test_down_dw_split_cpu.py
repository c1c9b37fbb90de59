"""NumPy emulation of the down-projection weight gradient on split-fp16 MFMA (csrc/outres_tn_split.hip, one block,
transposed store): the packed kernel with the roles swapped,

    dW_down^T[d][f] = sum_t g2[t][d] h[t][f]

    g2[:, d] 2^s(d) = xh + xl / 2048       the GRADIENT is the plane-image operand: one power of two per column d
    h 2^S = gh + gl / 2048                 the ACTIVATION (SwiGLU output, 768 columns) is the raw operand under the running
                                           exponent of a wave's sixteen columns

through `emulate_split` of tests/test_outres_tn_split_cpu.py (the arithmetic is that file's; only what plays x and g
changed).  The gradient's token rows are scaled, which is what a per-column exponent has to live with: a row far below its
column's largest keeps fewer bits of its own, while the error is measured against max |g2| max |h|.

Inputs: K = 8192 in one range, 48 columns of h = silu(a) b with a, b ~ N(0, 1) times 2^(-3 .. 3) per column, g2 ~ N(0, 1)
times 2^(-6 .. 6) per column and per token row flat, log-uniform over 1e-6 .. 1, on a geometric ramp 1e-8 -> 1e3 and
1e3 -> 1e-8, 1e-30, and flat with every seventh token row exactly zero; fp16 subnormal planes kept and flushed.

Criterion: the split form's figure is at most 2 x that of fp32 operands summed in pieces of 32 (the rule of the existing
file).  Measured here (subnormals kept / flushed): flat 0.76 / 0.76, loguniform 1.22 / 1.41, rising 1.12 / 1.12, falling
1.01 / 0.98, tiny 0.94 / 0.94, zero rows 1.54 / 1.54 x the fp32 operands' figure (which is 7.1e-8 .. 1.8e-6)."""
import numpy as np
import pytest

from tests.test_outres_tn_split_cpu import D, emulate_fp32, emulate_split, figure

K, V = 8192, 48
KINDS = ("flat", "loguniform", "rising", "falling", "tiny", "zerorows")


def _rows(kind, rng):
    if kind in ("flat", "zerorows"):
        r = np.ones(K)
        if kind == "zerorows":
            r[::7] = 0.0
        return r
    if kind == "loguniform":
        return 10.0 ** rng.uniform(-6, 0, K)
    if kind == "rising":
        return 10.0 ** np.linspace(-8, 3, K)
    if kind == "falling":
        return 10.0 ** np.linspace(3, -8, K)
    assert kind == "tiny"
    return np.full(K, 1e-30)


@pytest.fixture(scope="module")
def results():
    out = {}
    for i, kind in enumerate(KINDS):
        rng = np.random.default_rng(300 + i)
        g2 = (rng.standard_normal((K, D)) * np.exp2(rng.integers(-6, 7, D))[None, :] * _rows(kind, rng)[:, None]).astype(np.float32)
        a, b = rng.standard_normal((K, V)), rng.standard_normal((K, V))
        h = (a / (1.0 + np.exp(-a)) * b * np.exp2(rng.integers(-3, 4, V))[None, :]).astype(np.float32)
        rec = {}
        for flush in (False, True):
            got, moves = emulate_split(g2, h, flush)
            rec[flush] = (figure(got, g2, h), figure(emulate_fp32(g2, h, flush), g2, h), bool(np.isfinite(got).all()), got)
        out[kind] = rec
        print(f"{kind:11s} fp32 {rec[False][1]:.3e} / {rec[True][1]:.3e}   split {rec[False][0]:.3e} / {rec[True][0]:.3e}"
              f"   ratio {rec[False][0] / rec[False][1]:.2f} / {rec[True][0] / rec[True][1]:.2f}   (kept / flushed)")
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_split_within_twice_the_fp32_operands(results, kind):
    for flush in (False, True):
        split, fp32, finite, _ = results[kind][flush]
        assert finite and split <= 2.0 * fp32, (kind, flush, split, fp32)


def test_transposed_output_is_the_down_projection_gradient(results):
    """what the kernel's transposed store leaves in a slab is (h^T g2), row-major"""
    rng = np.random.default_rng(300)
    g2 = (rng.standard_normal((K, D)) * np.exp2(rng.integers(-6, 7, D))[None, :]).astype(np.float32)
    a, b = rng.standard_normal((K, V)), rng.standard_normal((K, V))
    h = (a / (1.0 + np.exp(-a)) * b * np.exp2(rng.integers(-3, 4, V))[None, :]).astype(np.float32)
    got = results["flat"][False][3].T
    ref = h.astype(np.float64).T @ g2.astype(np.float64)
    assert got.shape == (V, D)
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(g2).max() * np.abs(h).max()
