"""pydynet_amd/core/fused/smooth_loss.py, the float64 statement of cross entropy with label_smoothing and z_loss, against CPU
torch.nn.functional.cross_entropy(label_smoothing=, ignore_index=) in float64 and its autograd: 'none', 'sum' and 'mean', each
with and without ignore_index, eps in {0.1, 1.0}; the z-loss term against torch autograd of lam * logsumexp^2; the three-term
decomposition the lm_head node is built on against the direct formula; the argument rules.  count == 0 is left out of the
torch comparison (torch gives NaN, this project 0) and checked on its own."""
import numpy as np
import pytest

from pydynet_amd.core.fused import smooth_loss as S

torch = pytest.importorskip("torch")

ROWS, V = 23, 11


def _problem(ignore_index):
    rng = np.random.default_rng(7)
    z = 2.0 * rng.standard_normal((ROWS, V))
    t = rng.integers(1 if ignore_index == 0 else 0, V, ROWS)
    if ignore_index is not None:
        t = np.where(rng.random(ROWS) < 0.4, ignore_index, t)
    return z, t, rng.standard_normal(ROWS)


@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("ignore_index", [None, -100, 0])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_label_smoothing_against_torch(reduction, ignore_index, eps):
    z, t, u = _problem(ignore_index)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    kw = {} if ignore_index is None else {"ignore_index": ignore_index}
    ref = torch.nn.functional.cross_entropy(zt, torch.tensor(t), reduction=reduction, label_smoothing=eps, **kw)
    up = u if reduction == "none" else 0.7
    (ref * torch.tensor(up, dtype=torch.float64)).sum().backward()
    loss, d = S.cross_entropy(z, t, eps, 0.0, ignore_index, reduction, up)
    np.testing.assert_allclose(loss, ref.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(d, zt.grad.numpy(), rtol=1e-13, atol=1e-13)
    if reduction == "none":
        np.testing.assert_array_equal(loss, S.rows(z, t, eps, 0.0, ignore_index))
        valid = np.ones(ROWS, bool) if ignore_index is None else t != ignore_index
        assert not loss[~valid].any() and not d[~valid].any()


@pytest.mark.parametrize("ignore_index", [None, -100])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_z_loss_against_torch_autograd(reduction, ignore_index):
    z, t, u = _problem(ignore_index)
    eps, lam = 0.3, 0.05
    valid = torch.tensor(np.ones(ROWS, bool) if ignore_index is None else t != ignore_index)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    kw = {} if ignore_index is None else {"ignore_index": ignore_index}
    rows = torch.nn.functional.cross_entropy(zt, torch.tensor(t), reduction="none", label_smoothing=eps, **kw)
    rows = rows + torch.where(valid, lam * torch.logsumexp(zt, 1) ** 2, torch.zeros(ROWS, dtype=torch.float64))
    ref = rows if reduction == "none" else (rows.sum() if reduction == "sum" else rows.sum() / valid.sum())
    up = u if reduction == "none" else -1.3
    (ref * torch.tensor(up, dtype=torch.float64)).sum().backward()
    loss, d = S.cross_entropy(z, t, eps, lam, ignore_index, reduction, up)
    np.testing.assert_allclose(loss, ref.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(d, zt.grad.numpy(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("eps,lam", [(0.3, 0.0), (0.0, 0.05), (0.3, 0.05), (1.0, 2.0)])
@pytest.mark.parametrize("ignore_index", [None, -100, 0])
def test_three_term_decomposition(ignore_index, eps, lam):
    z, t, u = _problem(ignore_index)
    valid = np.ones(ROWS, bool) if ignore_index is None else t != ignore_index
    u = np.where(valid, u, np.nan)                        # an ignored row's upstream number may hold anything
    direct = S.dlogits(z, t, u, eps, lam, ignore_index)
    np.testing.assert_allclose(S.dlogits_decomposed(z, t, u, eps, lam, ignore_index), direct, rtol=1e-13, atol=1e-15)
    assert np.isfinite(direct).all() and not direct[~valid].any()
    up, c, e = S.coefficients(S._lse(z), valid, u, eps, lam, V)
    assert not up[~valid].any() and not c[~valid].any() and not e[~valid].any()
    # the lm_head form of the two correction terms: no pass over the logits
    rng = np.random.default_rng(3)
    x, w, b = rng.standard_normal((ROWS, 5)), rng.standard_normal((5, V)), rng.standard_normal(V)
    zz = x @ w + b
    value, dx, dW, db = S.linear_cross_entropy(x, w, b, t, eps, lam, ignore_index, "none", u)
    wsum, bsum = S.weight_sums(w, b)
    np.testing.assert_allclose((x @ wsum + bsum) / V, zz.mean(1), rtol=1e-13, atol=1e-13)
    up, c, e = S.coefficients(S._lse(zz), valid, u, eps, lam, V)
    from pydynet_amd.core.fused import row_loss
    _, dx0, dW0, db0 = row_loss.linear_cross_entropy(x, w, b, np.where(valid, t, -1), up, -1)
    ts = np.where(valid, t, 0)
    hot = np.zeros((ROWS, V))
    hot[np.arange(ROWS), ts] = c
    np.testing.assert_allclose(dx0 + c[:, None] * w[:, ts].T - e[:, None] * wsum[None, :], dx, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(dW0 + x.T @ hot - (e[:, None] * x).sum(0)[:, None], dW, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(db0 + hot.sum(0) - e.sum(), db, rtol=1e-12, atol=1e-13)


def test_rules():
    z, t, u = _problem(-100)
    for bad in ((-0.1, 0.0), (1.5, 0.0), (0.0, -1.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError):
            S.rows(z, t, *bad)
    with pytest.raises(IndexError):
        S.rows(z, np.where(np.arange(ROWS) == 3, V, t), 0.1, 0.0, -100)
    with pytest.raises(IndexError):
        S.rows(z, np.where(np.arange(ROWS) == 3, -1, t), 0.1, 0.0, -100)      # negative targets do not wrap
    # no row left: loss 0 and every gradient 0, under 'mean' too
    for reduction in ("mean", "sum"):
        loss, d = S.cross_entropy(z, np.full(ROWS, -100), 0.3, 0.05, -100, reduction, 2.0)
        assert loss == 0.0 and not d.any()
    # 'mean' averages both terms over the remaining rows
    rows = S.rows(z, t, 0.3, 0.05, -100)
    assert S.cross_entropy(z, t, 0.3, 0.05, -100, "mean")[0] == pytest.approx(rows.sum() / (t != -100).sum(), rel=1e-14)
