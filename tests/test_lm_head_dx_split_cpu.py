"""The arithmetic of the split-fp16 lm_head input gradient (csrc/lm_head_dx_split.hip) in NumPy, against float64.

    u[t][d] = sum_v e[t][v] W[d][v],  e = exp(logit - rowmax),  Z = sum_v e,  dx[t] = gscale (u[t] / Z[t] - W[:, target[t]])

The kernel forms e in fp32 from the fp32 logits (Z from the unsplit e), scales it by 2^s and splits it into two fp16 planes,
e 2^s = eh + el / 2048; every output column d (a row of W as stored) gets its own power of two (largest magnitude into
[2^8, 2^9)) and the same split; u 2^(s + s(d)) = eh wh + (eh wl + el wh) / 2048 -- fp16 products are exact in fp32, the sums
are fp32 -- and the scales leave in one ldexp.  `_shift` / `_planes` are those of the forward's test.

Why s = 15 and not the forward's 8: e lies in (0, 1] with thousands of small terms per row; at s = 8 everything below 2^-22
is an fp16 subnormal after scaling, and if the matrix pipe or a conversion flushes those the row error grows 18 x.  At
s = 15 (largest plane value 2^15, largest residual 2^15: both inside fp16) the result does not depend on it.  Why fp16 and
not bf16: 8 significand bits per plane leave 16, not 22.

Inputs: default_rng(9), x ~ N(0, 1), w ~ 0.05 N(0, 1), b ~ 0.1 N(0, 1), 256 rows, V = 32000; row 7 with all probability on
its target, row 8 scaled by 8 (sharp), row 9 by 0.01 (flat), w[17, :] *= 1e-6.  The logits are the fp32 `x @ w + b`; the
float64 reference is formed FROM THOSE fp32 logits.

What is asserted.  Unnormalised product, worst row error / the row's largest entry: the three-product fp16 form at s = 15,
subnormals kept AND flushed, is within 2 x the figure of an fp32 BLAS product of the same fp32 e (the factor only allows a
different summation order); s = 8 flushed and bf16 are not.  dx itself, max |err| / (gscale max |W|) per row (u / Z is a
convex combination of W's columns, so that is dx's natural scale; row 7's true gradient is ~1e-16 and a row-relative figure
would measure nothing there): split <= 2 x fp32 BLAS, and the same per output column at gscale max |W[d, :]| (covers
w[17]).  Measured here: product 4.23e-7 (fp32 BLAS), 4.42e-7 (fp16, s = 8 / 12 / 15 kept; s = 15 flushed), 7.93e-6 / 6.81e-7
(s = 8 / 12 flushed), 4.42e-6 (bf16); dx 1.14e-7 for fp32 BLAS and every passing fp16 form (the common fp32 exp and Z
dominate)."""
import numpy as np
import pytest

from tests.test_lm_head_split_cpu import _planes, _shift

K, V, ROWS = 288, 32000, 256
S_KERNEL = 15                                            # LD_ES of csrc/lm_head_dx_split.hip


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((ROWS, K), dtype=np.float32)
    w = (0.05 * rng.standard_normal((K, V))).astype(np.float32)
    b = (0.1 * rng.standard_normal(V)).astype(np.float32)
    t = rng.integers(0, V, ROWS)
    x[7] = 40.0 * w[:, t[7]] / np.linalg.norm(w[:, t[7]])
    x[8] *= np.float32(8.0)
    x[9] *= np.float32(0.01)
    w[17, :] *= np.float32(1e-6)
    logits = (x @ w + b).astype(np.float32)
    m = logits.max(1)
    e = np.exp(logits - m[:, None]).astype(np.float32)  # what the kernel forms, in fp32
    z = e.sum(1, dtype=np.float32)
    l64 = logits.astype(np.float64)
    e64 = np.exp(l64 - l64.max(1)[:, None])
    w64 = w.astype(np.float64)
    u_ref = e64 @ w64.T
    gscale = 1.0 / ROWS
    dx_ref = gscale * (u_ref / e64.sum(1)[:, None] - w64[:, t].T)
    return dict(w=w, t=t, e=e, z=z, u_ref=u_ref, dx_ref=dx_ref, gscale=gscale)


def split_product(e, w, s, fmt="fp16", ftz=False):
    """u = e @ w.T from the planes of e 2^s and of W's rows at their own power of two"""
    sw = _shift(np.abs(w).max(1))
    eh, el, up = _planes(e, np.int32(s), fmt, ftz)
    wh, wl, _ = _planes(w, sw[:, None], fmt, ftz)
    acc0 = eh @ wh.T                                     # float32 products of exactly representable factors, float32 sums
    acc1 = eh @ wl.T + el @ wh.T
    return np.ldexp(acc0 + acc1 / up, -(s + sw[None, :])).astype(np.float32)


def _row_err(u, u_ref):
    return float((np.abs(u.astype(np.float64) - u_ref).max(1) / np.abs(u_ref).max(1)).max())


def _dx(u, d):
    return (np.float32(d["gscale"]) * (u / d["z"][:, None] - d["w"][:, d["t"]].T)).astype(np.float32)


def _dx_err(dx, d):
    """worst row at the scale gscale max |W|, worst column at gscale max |W[d, :]|"""
    err = np.abs(dx.astype(np.float64) - d["dx_ref"])
    wmax = np.abs(d["w"].astype(np.float64))
    return float(err.max() / (d["gscale"] * wmax.max())), float((err.max(0) / (d["gscale"] * wmax.max(1))).max())


@pytest.mark.parametrize("ftz", [False, True])
def test_three_fp16_products_at_the_kernels_scale_are_at_fp32_accuracy(data, ftz):
    d = data
    u32 = d["e"] @ d["w"].T
    u = split_product(d["e"], d["w"], S_KERNEL, "fp16", ftz)
    e_split, e_f32 = _row_err(u, d["u_ref"]), _row_err(u32, d["u_ref"])
    print(f"product, worst row error / row max: fp16 x 3 s={S_KERNEL} ftz={ftz} {e_split:.3e}, fp32 BLAS {e_f32:.3e}")
    assert e_split <= 2.0 * e_f32, (e_split, e_f32)
    (r, c), (r32, c32) = _dx_err(_dx(u, d), d), _dx_err(_dx(u32, d), d)
    print(f"dx, max |err| / (gscale max |W|): rows {r:.3e} (fp32 BLAS {r32:.3e}), columns at their own scale {c:.3e} ({c32:.3e})")
    assert r <= 2.0 * r32, (r, r32)
    assert c <= 2.0 * c32, (c, c32)


def test_the_forwards_scale_depends_on_subnormal_handling(data):
    d = data
    e_f32 = _row_err(d["e"] @ d["w"].T, d["u_ref"])
    kept = _row_err(split_product(d["e"], d["w"], 8, "fp16", False), d["u_ref"])
    flushed = _row_err(split_product(d["e"], d["w"], 8, "fp16", True), d["u_ref"])
    print(f"product at s = 8: subnormals kept {kept:.3e}, flushed {flushed:.3e}, fp32 BLAS {e_f32:.3e}")
    assert kept <= 2.0 * e_f32
    assert not flushed <= 2.0 * e_f32


def test_three_bf16_products_are_not(data):
    d = data
    e_f32 = _row_err(d["e"] @ d["w"].T, d["u_ref"])
    e_bf = _row_err(split_product(d["e"], d["w"], S_KERNEL, "bf16"), d["u_ref"])
    print(f"product, bf16 x 3: {e_bf:.3e}, fp32 BLAS {e_f32:.3e}")
    assert not e_bf <= 2.0 * e_f32


def test_planes_stay_inside_fp16(data):
    eh, el, _ = _planes(data["e"], np.int32(S_KERNEL), "fp16", False)
    assert np.isfinite(eh).all() and np.isfinite(el).all()
    assert eh.max() == 2.0 ** S_KERNEL and np.abs(el).max() <= 2.0 ** 15
