"""The kernels behind the rest of the reference's surface -- pooling / im2col / col2im, the RNN and LSTM cell halves, the
persistent GRU, last-axis LayerNorm and the gated sigmoid, and everything float64 -- at the shapes where their index math,
grid caps, template choices and tails actually turn, each against a plain float64 (np.longdouble for the float64 products)
NumPy statement of the reference program's formula (tests/generic_kernels_ref.py; nothing there calls this package).

Every check is a `check_*(dev)` registered through `device_variants`: it runs on the MI355X under `-m gpu` and on the NumPy
emulation of the C ABI otherwise, so the references and criteria are exercised on a CPU-only box as well.  Each section's
docstring names the kernel file and the branch or cap its shapes were chosen to reach."""
import numpy as np
import pytest

from tests import generic_kernels_ref as ref
from tests.conftest import device_variants

F32 = np.float32
RT, AT = 2e-5, 2e-6                      # the stream tolerance of tests/test_kernels_gpu.py
U32, U64 = 2.0 ** -24, 2.0 ** -53       # unit round-off of float32 / float64


def _env(dev):
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.cuda import Device
    return hp, _lib.lib(), Device(dev)


def _ints(rng, shape, lo=-3, hi=3):
    """Small integers stored as float32: every sum of a few hundred of them is exact, and ties are everywhere."""
    return rng.integers(lo, hi + 1, shape).astype(F32)


def _normwise(got, want, what):
    """The criterion of tests/test_misc_layers.py."""
    a, r = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert a.shape == r.shape, (what, a.shape, r.shape)
    err = float(np.linalg.norm(a - r))
    assert err <= 1e-4 * float(np.linalg.norm(r)) + 1e-6, (what, err, float(np.linalg.norm(r)))


def _close(got, want, rtol, atol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~(np.abs(got - want) <= atol + rtol * np.abs(want))
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, np.abs(got - want), 0))), got.shape)
        raise AssertionError((what, "elements off", int(bad.sum()), "worst at", i, float(got[i]), float(want[i])))


# =====================================================================================================================
# 1. pooling, im2col, col2im
# =====================================================================================================================
SWEEP = [(2, 2, 0), (2, 2, 1), (3, 1, 1), (3, 2, 0), (3, 2, 1), (2, 3, 0), (5, 1, 2), (1, 1, 0), (3, 3, 2), (2, 1, 2)]
PLANES = [(3, 5, 13, 9), (3, 5, 32, 17)]           # 15 planes: neither one nor a multiple of any grid; H != W
LARGE = (9, 30, 64, 64, 3, 1, 1)                   # 1,105,920 pixels / outputs: above the 4096 x 256 threads of grid1d


def _pool_raw(hp, L, x, dy, k, s, p, mode):
    N, C, H, W = x.shape
    oh, ow = ref.out_size(H, W, k, s, p)
    X, DY = hp.from_numpy(x), hp.from_numpy(dy)
    Y, DX = hp.full((N, C, oh, ow), np.nan, F32), hp.full(x.shape, np.nan, F32)
    m = 0 if mode == "max" else 1
    L.call("pdn_pool2d_fwd_f32", X._ptr, N, C, H, W, k, s, p, m, Y._ptr, hp.stream())
    L.call("pdn_pool2d_bwd_f32", X._ptr, Y._ptr, DY._ptr, N, C, H, W, k, s, p, m, DX._ptr, hp.stream())
    return Y.get(), DX.get()


def _check_pool_case(hp, L, rng, shape, k, s, p, modes=("max", "avg"), need_ties=True):
    x = _ints(rng, shape)
    if p > 0:                                       # a negative corner: window (0, 0) reaches the padding, whose zero alone wins
        x[0, 0, :k, :k] = -1 - (np.arange(k)[:, None] + np.arange(k)) % 3
    oh, ow = ref.out_size(shape[2], shape[3], k, s, p)
    if "max" in modes and need_ties:
        tied, pad_wins = ref.tie_census(x, k, s, p)
        assert k == 1 or tied > 0, ("no tied window: the tie rule is not exercised", shape, k, s, p)
        assert p == 0 or pad_wins > 0, ("no window that only the padding zero wins", shape, k, s, p)
    for mode in modes:
        # max: integer gradients of both signs (sums of <= k*k of them are exact).  avg: positive ones, so that the
        # k*k-term sum of rounded quotients has no cancellation and a relative bound is meaningful
        dy = _ints(rng, shape[:2] + (oh, ow)) if mode == "max" else _ints(rng, shape[:2] + (oh, ow), 1, 3)
        y, dx = _pool_raw(hp, L, x, dy, k, s, p, mode)
        y_ref, dx_ref = ref.pool_fwd(x, k, s, p, mode), ref.pool_bwd(x, dy, k, s, p, mode)
        what = (shape, k, s, p, mode)
        if mode == "max" or (k * k) & (k * k - 1) == 0:
            assert np.array_equal(y, y_ref), what + ("y",)
            assert np.array_equal(dx, dx_ref), what + ("dx",)
        else:
            # k*k is not a power of two: the quotient rounds (once forward: u = 6e-8; backward a same-sign sum of <= k*k
            # rounded quotients, at most k*k * u = 1.5e-6 for k = 5): rtol 2e-6, exact zeros where no window reaches
            _close(y, y_ref, 2e-6, 0.0, what + ("y",))
            _close(dx, dx_ref, 2e-6, 0.0, what + ("dx",))


def check_pool2d_shape_sweep(dev):
    """csrc/conv.hip pool2d_fwd_kernel / pool2d_bwd_kernel: the overlapping-window branch of the backward (k != s, also
    k < s where pixels stay uncovered), pad > 0 (the padding zero takes part in max and may win), pad >= k, H != W, several
    planes; ties pinned by integer inputs (every position equal to the window's maximum gets the gradient)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(101)
    with device:
        for shape in PLANES:
            for k, s, p in SWEEP:
                _check_pool_case(hp, L, rng, shape, k, s, p)


def check_pool2d_grid_caps(dev):
    """csrc/conv.hip grid1d caps the forward grid at 4096 workgroups (1,048,576 threads): 1,105,920 outputs turn its
    grid-stride loop.  pool2d_bwd_kernel takes one plane per workgroup and at most 2^20 workgroups: 1,050,589 planes make
    its plane loop turn, on the overlapping-window branch."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(102)
    N, C, H, W, k, s, p = LARGE
    with device:
        _check_pool_case(hp, L, rng, (N, C, H, W), k, s, p)
        _check_pool_case(hp, L, rng, (1031, 1019, 2, 3), 2, 1, 0, modes=("max",))


def _check_im2col_case(hp, L, rng, shape, k, s, p, variants=None):
    N, C, H, W = shape
    oh, ow = ref.out_size(H, W, k, s, p)
    M, ckk = oh * ow, C * k * k
    x = _ints(rng, shape)
    X = hp.from_numpy(x)
    want = ref.windows(x, k, s, p).reshape(N, ckk, M)
    kp = (ckk + 1 + 3) // 4 * 4                     # the padded contraction of fused.conv2d (room for the ones row)
    for rows, ones_row in variants or ((ckk, 0), (ckk + 1, 1), (kp, 0), (kp, 1)):
        col = hp.full((N, rows, M), -77.0, F32)     # sentinel: every row must be written
        L.call("pdn_im2col2d_f32", X._ptr, N, C, H, W, k, s, p, col._ptr, rows, ones_row, hp.stream())
        got = col.get()
        what = (shape, k, s, p, rows, ones_row)
        assert np.array_equal(got[:, :ckk], want), what
        if ones_row:
            assert np.all(got[:, ckk] == 1.0), what + ("ones row",)
        assert np.all(got[:, ckk + (1 if ones_row else 0):] == 0.0), what + ("zero rows",)
        # col2im of the same padded layout: the padding rows hold garbage and must not be read
        dcol = _ints(rng, (N, rows, M))
        dcol[:, ckk:] = np.nan
        DC, DX = hp.from_numpy(dcol), hp.full(shape, np.nan, F32)
        L.call("pdn_col2im2d_f32", DC._ptr, N, C, H, W, k, s, p, DX._ptr, rows, hp.stream())
        dx_ref = ref.scatter_windows(dcol[:, :ckk].astype(np.float64).reshape(N, C, k, k, oh, ow), H, W, k, s, p)
        assert np.array_equal(DX.get(), dx_ref), what + ("col2im",)


def check_im2col_col2im_shape_sweep(dev):
    """csrc/conv.hip im2col2d_kernel / col2im2d_kernel: k in {1, 2, 3, 5}, s up to 3, H != W, p >= k; col_rows above
    C*k*k, whose rows the extra workgroup c == C writes (ones then zeros) and col2im must skip; bit-exact copies / exact
    integer sums."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(103)
    with device:
        for shape in PLANES:
            for k, s, p in SWEEP:
                _check_im2col_case(hp, L, rng, shape, k, s, p)


def check_im2col_col2im_large_and_refusals(dev):
    """csrc/conv.hip: 9.95 M im2col outputs; N*C*H*W = 1,105,920 > the 1,048,576 threads grid1d gives col2im2d_kernel (its
    grid-stride loop turns).  The launch uses N as gridDim.y: N > 65535 is refused, as is a col_rows with no room."""
    from pydynet_amd._lib import HipLibraryError
    hp, L, device = _env(dev)
    rng = np.random.default_rng(104)
    N, C, H, W, k, s, p = LARGE
    with device:
        _check_im2col_case(hp, L, rng, (N, C, H, W), k, s, p, variants=((C * k * k + 2, 1),))
        x, col = hp.zeros((65536, 1, 1, 1), F32), hp.zeros((65536, 1, 1), F32)
        with pytest.raises(HipLibraryError):
            L.call("pdn_im2col2d_f32", x._ptr, 65536, 1, 1, 1, 1, 1, 0, col._ptr, 1, 0, hp.stream())
        with pytest.raises(HipLibraryError):                                   # ones_row needs col_rows >= C*k*k + 1
            L.call("pdn_im2col2d_f32", x._ptr, 4, 1, 1, 1, 1, 1, 0, col._ptr, 1, 1, hp.stream())
        L.call("pdn_im2col2d_f32", x._ptr, 65535, 1, 1, 1, 1, 1, 0, col._ptr, 1, 0, hp.stream())   # the largest N it takes


def check_pool_and_conv_through_the_tape(dev):
    """F.max_pool2d / F.avg_pool2d with k != s and pad > 0 (fused.pool2d -> csrc/conv.hip) and F.conv2d on a shape the
    direct kernels reject (O = 70 > 64 output channels: pdn_conv2d_direct_supported == 0), so im2col + GEMM + col2im run;
    forward and backward() against the same float64 statements."""
    import pydynet_amd as pdn
    import pydynet_amd.nn.functional as F
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    hp, L, device = _env(dev)
    rng = np.random.default_rng(105)
    T = lambda a, g=False: pdn.Tensor(a, dtype=F32, device=dev, requires_grad=g)
    for shape in ((3, 5, 13, 9), (2, 3, 32, 17)):
        for fn, mode in ((F.max_pool2d, "max"), (F.avg_pool2d, "avg")):
            for k, s, p in ((3, 2, 1), (3, 1, 1), (2, 3, 1), (2, 1, 1)):
                Graph.clear()
                x = _ints(rng, shape)
                oh, ow = ref.out_size(shape[2], shape[3], k, s, p)
                gp = _ints(rng, shape[:2] + (oh, ow)) if mode == "max" else _ints(rng, shape[:2] + (oh, ow), 1, 3)
                X = T(x, True)
                out = fn(X, k, s, p)
                assert type(out).__name__ == "pool2d" and out.shape == shape[:2] + (oh, ow)
                (out * T(gp)).sum().backward()
                y_ref, dx_ref = ref.pool_fwd(x, k, s, p, mode), ref.pool_bwd(x, gp, k, s, p, mode)
                if mode == "max" or k == 2:
                    assert np.array_equal(out.numpy(), y_ref) and np.array_equal(X.grad.get(), dx_ref), (shape, mode, k, s, p)
                else:                                                          # k*k = 9: the quotient rounds (see above)
                    _close(out.numpy(), y_ref, 2e-6, 0.0, (shape, mode, k, s, p, "y"))
                    _close(X.grad.get(), dx_ref, 2e-6, 0.0, (shape, mode, k, s, p, "dx"))
    for (N, C, H, W, O, k, s, p) in ((3, 20, 20, 18, 70, 3, 1, 1), (2, 7, 15, 11, 70, 5, 2, 2), (2, 20, 15, 11, 70, 3, 2, 1)):
        Graph.clear()
        assert L.query("pdn_conv2d_direct_supported", C, H, W, O, k, s, p) == 0
        x, w, b = _ints(rng, (N, C, H, W)), _ints(rng, (O, C, k, k), -1, 1), _ints(rng, (1, O, 1, 1))
        oh, ow = ref.out_size(H, W, k, s, p)
        g = _ints(rng, (N, O, oh, ow))
        X, Wt, Bt = T(x, True), T(w, True), T(b, True)
        node = F.conv2d(X, Wt, p, s, Bt)
        assert type(node) is fused.conv2d and node._pending is None          # not deferred: no fused chain takes it
        assert node._direct == 0 and node._colp is not None                     # the im2col + GEMM route ran
        (node * T(g)).sum().backward()
        # integer operands: every product and partial sum is an integer below 2^24, exact in float32 in any order
        y_ref, dx_ref, dw_ref, db_ref = ref.conv2d_ref(x, w, b.reshape(-1), g, s, p)
        for got, want, name in ((node.numpy(), y_ref, "y"), (X.grad.get(), dx_ref, "dx"), (Wt.grad.get(), dw_ref, "dw"),
                                (Bt.grad.get().reshape(-1), db_ref, "db")):
            assert np.array_equal(got, want), ((N, C, H, W, O, k, s, p), name, float(np.abs(got - want).max()))


# =====================================================================================================================
# 2. RNN and LSTM cell halves
# =====================================================================================================================
CELL_SIZES = [(1, 1), (3, 6), (70, 33), (257, 100), (4099, 300)]      # the last: 1,229,700 elements > rc_grid's 4096 x 256


def _saturate(lin, rng):
    """Scale the leading third of the rows to +-20, +-60 and +-100; returns the magnitudes (0 = left alone)."""
    mag = np.zeros(lin.shape, F32)
    nb = lin.shape[0] // 3
    if nb:
        mag[:nb] = rng.choice(np.array([20, 60, 100], F32), (nb, lin.shape[1]))
        lin[:nb] = mag[:nb] * rng.choice(np.array([-1, 1], F32), (nb, lin.shape[1]))
    return mag


def _check_saturated(got, want, mag, what):
    """Piecewise sigmoid / tanh at +-20 / +-60 / +-100: finite, equal to float64 to the spacing of float32 in [1, 2)
    (2^-23: the forms are 1 - q or q - 1 with q rounded in [0.5, 2]), and at +-100 exactly 1, -1, or within 2^-24 of 0."""
    assert np.isfinite(got).all(), what
    sat = mag > 0
    assert np.all(np.abs(got[sat].astype(np.float64) - want[sat]) <= 2 * U32), what
    far = mag == 100
    r = np.rint(want[far])                                                  # 1, -1 or 0 (sigmoid of -100)
    assert np.all(np.where(r != 0, got[far] == r, np.abs(got[far]) <= U32)), what


def check_rnn_cell_kernels(dev):
    """csrc/rnn_cell.hip rnn_cell_fwd/bwd_kernel (nn/modules/rnn.py:35-47): both activations, sizes up to past the grid cap
    of rc_grid (grid-stride loop), saturated tanh (piecewise form), and relu exactly at 0 (+0 and -0), where the gradient
    passes because out == x."""
    hp, L, device = _env(dev)
    with device:
        for B, H in CELL_SIZES:
            rng = np.random.default_rng(B * 1000 + H)
            n = B * H
            lin = (2 * rng.standard_normal((B, H))).astype(F32)
            mag = _saturate(lin, rng)
            dy = rng.standard_normal((B, H)).astype(F32)
            # tanh
            LIN, DY, Y = hp.from_numpy(lin), hp.from_numpy(dy), hp.full((B, H), np.nan, F32)
            L.call("pdn_rnn_cell_fwd_f32", LIN._ptr, Y._ptr, n, 0, hp.stream())
            y_ref = np.tanh(lin.astype(np.float64))
            _close(Y.get(), y_ref, RT, AT, (B, H, "tanh"))
            _check_saturated(Y.get(), y_ref, mag, (B, H, "tanh saturated"))
            y32 = y_ref.astype(F32)                                         # the backward entry's inputs, made on the host
            Y32, DL = hp.from_numpy(y32), hp.full((B, H), np.nan, F32)
            L.call("pdn_rnn_cell_bwd_f32", LIN._ptr, Y32._ptr, DY._ptr, DL._ptr, n, 0, hp.stream())
            _close(DL.get(), (1 - y32.astype(np.float64) ** 2) * dy, 1e-4, 1e-6, (B, H, "dtanh"))
            assert np.isfinite(DL.get()).all()
            # relu, with exact zeros of both signs planted
            lin.reshape(-1)[::7] = 0.0
            lin.reshape(-1)[3::11] = -0.0
            LIN = hp.from_numpy(lin)
            L.call("pdn_rnn_cell_fwd_f32", LIN._ptr, Y._ptr, n, 1, hp.stream())
            y = np.maximum(0.0, lin.astype(np.float64))
            assert np.array_equal(Y.get(), y), (B, H, "relu")
            Y32 = hp.from_numpy(y.astype(F32))
            L.call("pdn_rnn_cell_bwd_f32", LIN._ptr, Y32._ptr, DY._ptr, DL._ptr, n, 1, hp.stream())
            got = DL.get()
            assert np.array_equal(got, np.where(y == lin, dy, 0)), (B, H, "drelu")
            zero = lin == 0
            assert zero.any() and np.array_equal(got[zero], dy[zero]), (B, H, "the gradient passes at 0")


def check_lstm_cell_kernels(dev):
    """csrc/rnn_cell.hip lstm_cell_fwd/bwd_kernel (nn/modules/rnn.py:244-262): the (b, j) index split at H not a power of
    two, B * H past the grid cap, saturated gates, and a backward whose dc' half (from later consumers) is not zero."""
    hp, L, device = _env(dev)
    with device:
        for B, H in CELL_SIZES:
            rng = np.random.default_rng(B * 1000 + H + 1)
            lin = (2 * rng.standard_normal((B, 4 * H))).astype(F32)
            mag = _saturate(lin, rng)
            c = rng.standard_normal((B, H)).astype(F32)
            G, TC, HC = hp.full((B, 4 * H), np.nan, F32), hp.full((B, H), np.nan, F32), hp.full((B, 2 * H), np.nan, F32)
            LIN, Cd = hp.from_numpy(lin), hp.from_numpy(c)
            L.call("pdn_lstm_cell_fwd_f32", LIN._ptr, Cd._ptr, G._ptr, TC._ptr, HC._ptr, B, H, hp.stream())
            gates, t, h, cn = ref.lstm_cell(lin, c)
            _close(G.get(), gates, RT, AT, (B, H, "gates"))
            _check_saturated(G.get(), gates, mag, (B, H, "gates saturated"))
            _close(TC.get(), t, RT, AT, (B, H, "tanh c'"))
            _close(HC.get()[:, :H], h, RT, AT, (B, H, "h'"))
            _close(HC.get()[:, H:], cn, RT, AT, (B, H, "c'"))
            assert np.isfinite(HC.get()).all() and np.isfinite(TC.get()).all()
            # backward: the entry's inputs (gates, tanh c') made on the host from float64, dc' from later consumers != 0
            g32, t32 = gates.astype(F32), t.astype(F32)
            dhc = rng.standard_normal((B, 2 * H)).astype(F32)
            DL, DC = hp.full((B, 4 * H), np.nan, F32), hp.full((B, H), np.nan, F32)
            DHC, G32, T32 = hp.from_numpy(dhc), hp.from_numpy(g32), hp.from_numpy(t32)
            L.call("pdn_lstm_cell_bwd_f32", DHC._ptr, G32._ptr, T32._ptr, Cd._ptr, DL._ptr, DC._ptr, B, H, hp.stream())
            dlin, dc = ref.lstm_cell_bwd(dhc[:, :H], dhc[:, H:], g32, t32, c)
            assert np.abs(dhc[:, H:]).min() > 0
            _close(DL.get(), dlin, 1e-4, 1e-6, (B, H, "dlin"))
            _close(DC.get(), dc, 1e-4, 1e-6, (B, H, "dc"))
            assert np.isfinite(DL.get()).all() and np.isfinite(DC.get()).all()


def check_lstm_rnn_modules_against_float64_unroll(dev):
    """nn.LSTM / nn.RNN (tanh, relu) at T = 7, B = 70, I = 20, H = 96 on the device -- fused.lstm_cell / fused.rnn_cell: two
    GEMMs + csrc/rnn_cell.hip per step -- against a float64 unroll of nn/modules/rnn.py, outputs, final states, dx and
    every parameter gradient."""
    import pydynet_amd as pdn
    import pydynet_amd.nn as nn
    from pydynet_amd.core.tensor import Graph
    T_, B, I, H = 7, 70, 20, 96
    rng = np.random.default_rng(7)
    t = lambda a, g=False: pdn.Tensor(a.astype(F32), dtype=F32, device=dev, requires_grad=g)
    x = rng.standard_normal((T_, B, I)).astype(F32)
    wo, whn, wcn = (rng.standard_normal(s).astype(F32) for s in ((T_, B, H), (1, B, H), (1, B, H)))
    Graph.clear()
    np.random.seed(11)
    lstm = nn.LSTM(I, H, dtype=F32)
    cell = lstm.cells[0]
    wx, wh, b = (np.array(p.data, copy=True) for p in (cell.Wx, cell.Wh, cell.bias))
    lstm = lstm.to(dev)
    X = t(x, True)
    o, (hn, cn) = lstm(X)
    ((o * t(wo)).sum() + (hn * t(whn)).sum() + (cn * t(wcn)).sum()).backward()
    r_out, r_h, r_c, r_dx, r_dwx, r_dwh, r_db = ref.lstm_sequence(x, wx, wh, b, wo, whn, wcn)
    _normwise(o.numpy(), r_out, "lstm out"); _normwise(hn.numpy()[0], r_h, "lstm hn"); _normwise(cn.numpy()[0], r_c, "lstm cn")
    _normwise(X.grad.get(), r_dx, "lstm dx")
    cell = lstm.cells[0]
    _normwise(cell.Wx.grad.get(), r_dwx, "lstm dWx"); _normwise(cell.Wh.grad.get(), r_dwh, "lstm dWh")
    _normwise(cell.bias.grad.get(), r_db, "lstm db")
    for act in ("tanh", "relu"):
        Graph.clear()
        np.random.seed(12)
        rnn = nn.RNN(I, H, nonlinearity=act, dtype=F32)
        cell = rnn.cells[0]
        wx, wh, b = (np.array(p.data, copy=True) for p in (cell.Wx, cell.Wh, cell.bias))
        rnn = rnn.to(dev)
        X = t(x, True)
        o, hn = rnn(X)
        (o * t(wo)).sum().backward()
        r_out, r_h, r_dx, r_dwx, r_dwh, r_db = ref.rnn_sequence(x, wx, wh, b, wo, act)
        _normwise(o.numpy(), r_out, f"rnn {act} out"); _normwise(hn.numpy()[0], r_h, f"rnn {act} hn")
        _normwise(X.grad.get(), r_dx, f"rnn {act} dx")
        cell = rnn.cells[0]
        _normwise(cell.Wx.grad.get(), r_dwx, f"rnn {act} dWx"); _normwise(cell.Wh.grad.get(), r_dwh, f"rnn {act} dWh")
        _normwise(cell.bias.grad.get(), r_db, f"rnn {act} db")


# =====================================================================================================================
# 3. GRU sequence
# =====================================================================================================================
def _gru_case(dev, T_, B, H, I, persistent):
    import pydynet_amd as pdn
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    rng = np.random.default_rng(1000 * T_ + B + H)
    names = ("x", "h0", "wx1", "wh1", "wx2", "wh2", "b1", "b2")
    arrs = dict(x=rng.standard_normal((T_, B, I)), h0=rng.standard_normal((B, H)),
                wx1=0.3 * rng.standard_normal((I, 2 * H)), wh1=0.3 * rng.standard_normal((H, 2 * H)),
                wx2=0.3 * rng.standard_normal((I, H)), wh2=0.3 * rng.standard_normal((H, H)),
                b1=0.1 * rng.standard_normal((2 * H,)), b2=0.1 * rng.standard_normal((H,)))
    arrs = {k: v.astype(F32) for k, v in arrs.items()}
    wo = rng.standard_normal((T_, B, H)).astype(F32)
    Graph.clear()
    ts = {k: pdn.Tensor(v, dtype=F32, device=dev, requires_grad=True) for k, v in arrs.items()}
    node = fused.gru_sequence(*(ts[k] for k in names))
    assert node._persistent == persistent, (T_, B, H, node._persistent)
    (node * pdn.Tensor(wo, dtype=F32, device=dev)).sum().backward()
    out_ref, grads_ref = ref.gru_sequence(*(arrs[k] for k in names), wo)
    _normwise(node.numpy(), out_ref, (T_, B, H, "out"))
    for k, g in zip(names, grads_ref):
        _normwise(ts[k].grad.get(), g, (T_, B, H, "d" + k))


def check_gru_sequence_against_float64_unroll(dev):
    """csrc/gru_seq.hip (the whole time loop in one launch, a wave owns 32 sequences; H = 32) against a float64 unroll of
    the reference's GRU formula: T = 1, B = 1, a B that crosses a 32-row group (33, 70), the ts_prediction batch 1568 over
    40 steps; the output and every gradient, h0's included.  One H = 48 case keeps the per-step path (gru_gates / gru_out
    kernels + GEMMs of fused.gru_sequence) on the same reference."""
    for T_, B in ((1, 1), (1, 70), (40, 1), (9, 33), (40, 1568)):
        _gru_case(dev, T_, B, 32, 3, True)
    _gru_case(dev, 9, 70, 48, 5, False)


# =====================================================================================================================
# 4. last-axis LayerNorm, gated sigmoid
# =====================================================================================================================
LN_COLS = [4, 64, 256, 260, 768, 1024, 1796, 2048]        # VPL = ceil(cols / 256): 1 1 1 2 3 4 8 8 -- plus 5, 6, 7 below
LN_COLS_MORE = [1280, 1536, 1792]                            # VPL 5, 6, 7
LN_ROWS = [1, 3, 17, 700]
EPS = 1e-5


def _ln_forward(hp, L, x, w, b):
    rows, cols = x.shape
    Y, MU, RS = hp.full((rows, cols), np.nan, F32), hp.full((rows,), np.nan, F32), hp.full((rows,), np.nan, F32)
    X, Wd, Bd = hp.from_numpy(x), hp.from_numpy(w), hp.from_numpy(b)
    L.call("pdn_layernorm_fwd_f32", X._ptr, Wd._ptr, Bd._ptr, Y._ptr, MU._ptr, RS._ptr, rows, cols, EPS, hp.stream())
    return Y.get(), MU.get(), RS.get()


def _ln_backward(hp, L, x, w, mu, rs, dy, res=None, dw0=None, db0=None, want_dw=True, want_db=True, accumulate=0):
    rows, cols = x.shape
    DX = hp.full((rows, cols), np.nan, F32)
    DW = hp.from_numpy(dw0.copy() if dw0 is not None else np.full(cols, np.nan, F32)) if want_dw else None
    DB = hp.from_numpy(db0.copy() if db0 is not None else np.full(cols, np.nan, F32)) if want_db else None
    ws, wsb = hp.workspace(L.query("pdn_layernorm_bwd_workspace_bytes", rows, cols)) if (want_dw or want_db) else (None, 0)
    X, Wd, MU, RS, DY = (hp.from_numpy(a) for a in (x, w, mu, rs, dy))
    RES = hp.from_numpy(res) if res is not None else None
    L.call("pdn_layernorm_bwd_f32", X._ptr, Wd._ptr, MU._ptr, RS._ptr, DY._ptr, RES._ptr if res is not None else None, DX._ptr,
           DW._ptr if want_dw else None, DB._ptr if want_db else None, accumulate, rows, cols, ws, wsb, hp.stream())
    return DX.get(), DW.get() if want_dw else None, DB.get() if want_db else None


def _column_sum_error_in_kernel_order(terms):
    """The error, against float64, of summing `terms` (rows, cols) over the rows in float32 in rowln_bwd_kernel's order
    (csrc/rownorm.hip): nb = min(ceil(rows / 16), 1024) workgroups of 4 waves, wave v of workgroup g adds rows
    4 g + v, + 4 nb, ... in sequence; a workgroup's partial is (w0 + w1) + (w2 + w3); rowln_reduce_kernel adds the
    partials in workgroup order."""
    rows, cols = terms.shape
    nb = min((rows + 15) // 16, 1024)
    per = -(-rows // (4 * nb))
    t = np.zeros((per * 4 * nb, cols), F32)
    t[:rows] = terms.astype(F32)
    t = t.reshape(per, nb, 4, cols)
    acc = np.zeros((nb, 4, cols), F32)
    for j in range(per):
        acc = acc + t[j]
    part = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    s = np.zeros(cols, F32)
    for g in range(nb):
        s = s + part[g]
    return float(np.abs(s.astype(np.float64) - terms.astype(np.float64).sum(0)).max())


def _check_layernorm_case(hp, L, rows, cols, rng, variants=True):
    what = (rows, cols)
    # a common offset: the two-pass variance matters.  The alternating +-1.5 keeps every row's spread near or above 1 also at
    # cols = 4, where four normal draws alone can fall within 0.05 of each other and rstd then magnifies the float32
    # rounding of the row mean (4e-6 at 100) past any fixed tolerance
    x = (100.0 + rng.standard_normal((rows, cols)) + 1.5 * (1 - 2 * (np.arange(cols) % 2))).astype(F32)
    mu_ref, rs_ref = ref.layernorm_stats(x, EPS)
    # (a) against pure float64.  The row mean is held in float32, whose spacing at 100 is 7.6e-6: no float32 kernel can
    #     give xhat to better than ~4e-6 absolute here, above the stream atol; the shift keeps |y| >= 4, where its rtol rules
    w = (1 + 0.25 * rng.standard_normal(cols)).astype(F32)
    b = (10 + rng.standard_normal(cols)).astype(F32)
    y, mu, rs = _ln_forward(hp, L, x, w, b)
    _close(y, ref.layernorm_fwd(x, w, b, mu_ref, rs_ref), RT, AT, what + ("y",))
    # the saved statistics.  The mean: a summation tree of depth d errs by at most d u mean|x| (first order).  The kernel's
    # tree: 2 additions inside a float4, VPL - 1 across a lane's float4s, log2 of the lanes that hold data, 1 division --
    # 3 u at cols = 4 (2.4 float32 spacings at 100), 16 u at cols = 2048.  The two-pass variance of exactly formed
    # differences is good to float32 round-off -> the stream rtol
    n4 = cols // 4
    depth = 2 + (-(-n4 // 64) - 1) + int(np.ceil(np.log2(min(64, n4)))) + 1
    assert np.all(np.abs(mu - mu_ref) <= 1.01 * depth * U32 * np.abs(x.astype(np.float64)).mean(-1)), what + ("mean",)
    _close(rs, rs_ref, RT, 0.0, what + ("rstd",))
    # (b) ordinary scale / shift of both signs, small |y| included: against the float64 formula at the statistics the
    #     kernel saved (their own accuracy is pinned above)
    w = rng.standard_normal(cols).astype(F32)
    b = rng.standard_normal(cols).astype(F32)
    y, mu, rs = _ln_forward(hp, L, x, w, b)
    _close(y, ref.layernorm_fwd(x, w, b, mu, rs), RT, AT, what + ("y at saved statistics",))
    # backward: mean / rstd are INPUTS of the entry -- float64 statistics rounded on the host
    mu32, rs32 = mu_ref.astype(F32), rs_ref.astype(F32)
    dy = rng.standard_normal((rows, cols)).astype(F32)
    dx_ref, dw_ref, db_ref = ref.layernorm_bwd(x, w, mu32, rs32, dy)
    extra = 0.0
    if rows > 16384:
        # 1024 partials of ~20 rows each, added in sequence, do not fit test_rmsnorm_fwd_bwd's atol of 1e-4 in float32:
        # measured on the host (float32 NumPy in the kernel's order against float64 NumPy, this seed) 4.1e-4 for dw and
        # 3.9e-4 for db at 20,001 x 128.  Four times the measured value is allowed on top (never the device's own output)
        xh = ((x - mu32[:, None]) * rs32[:, None]).astype(F32)
        extra = 4 * max(_column_sum_error_in_kernel_order(dy * xh), _column_sum_error_in_kernel_order(dy))
    dx, dw, db = _ln_backward(hp, L, x, w, mu32, rs32, dy)
    _close(dx, dx_ref, 1e-4, 1e-5, what + ("dx",))
    _close(dw, dw_ref, 1e-4, 1e-4 + extra, what + ("dw",))
    _close(db, db_ref, 1e-4, 1e-4 + extra, what + ("db",))
    if not variants:
        return
    res = rng.standard_normal((rows, cols)).astype(F32)
    dw0, db0 = rng.standard_normal(cols).astype(F32), rng.standard_normal(cols).astype(F32)
    dx, dw, db = _ln_backward(hp, L, x, w, mu32, rs32, dy, res=res, dw0=dw0, db0=db0, accumulate=1)
    _close(dx, dx_ref + res, 1e-4, 1e-5, what + ("dx + residual",))
    _close(dw, dw_ref + dw0, 1e-4, 1e-4 + extra, what + ("dw accumulated",))
    _close(db, db_ref + db0, 1e-4, 1e-4 + extra, what + ("db accumulated",))
    dx, dw, db = _ln_backward(hp, L, x, w, mu32, rs32, dy, res=res)                              # each flag alone
    _close(dx, dx_ref + res, 1e-4, 1e-5, what + ("dx + residual, no accumulate",))
    _close(dw, dw_ref, 1e-4, 1e-4 + extra, what + ("dw, residual, no accumulate",))
    _close(db, db_ref, 1e-4, 1e-4 + extra, what + ("db, residual, no accumulate",))
    dx, dw, db = _ln_backward(hp, L, x, w, mu32, rs32, dy, dw0=dw0, db0=db0, accumulate=1)
    _close(dx, dx_ref, 1e-4, 1e-5, what + ("dx, accumulate, no residual",))
    _close(dw, dw_ref + dw0, 1e-4, 1e-4 + extra, what + ("dw accumulated, no residual",))
    _close(db, db_ref + db0, 1e-4, 1e-4 + extra, what + ("db accumulated, no residual",))
    dx, dw, db = _ln_backward(hp, L, x, w, mu32, rs32, dy, want_dw=False, want_db=False)      # no workspace either
    _close(dx, dx_ref, 1e-4, 1e-5, what + ("dx alone",))
    dx, dw, db = _ln_backward(hp, L, x, w, mu32, rs32, dy, want_db=False)
    _close(dx, dx_ref, 1e-4, 1e-5, what + ("dx, only dw",))
    _close(dw, dw_ref, 1e-4, 1e-4 + extra, what + ("only dw",))


def check_layernorm_kernels(dev):
    """csrc/rownorm.hip rowln_fwd_kernel / rowln_bwd_kernel<VPL>: every VPL template 1..8 (cols / 4 lanes of float4, 64
    lanes a group), a partial last lane group (260, 1796), waves without a row (rows < 4), dx_residual and accumulate (each
    alone and together), null dw / db; 20,001 rows pass the 4096-workgroup forward grid (16,384 waves) and the backward's nb = 1024 cap, so both
    row loops turn.  Tolerances: tests/test_kernels_gpu.py::test_rmsnorm_fwd_bwd."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(401)
    with device:
        for cols in LN_COLS:
            for rows in LN_ROWS:
                _check_layernorm_case(hp, L, rows, cols, rng)
        for cols in LN_COLS_MORE:
            _check_layernorm_case(hp, L, 17, cols, rng, variants=False)
        _check_layernorm_case(hp, L, 20001, 128, rng)


def check_gated_sigmoid_kernels(dev):
    """csrc/rownorm.hip gated_sigmoid_fwd/bwd_kernel: n % 4 != 0 (the scalar tail loop, alone for n < 4), one full pass of
    float4 plus a tail, n past the 8192-workgroup cap (grid-stride loop); inputs across +-30 (exp(51) must not hurt)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(402)
    with device:
        for alpha in (1.702, 1.0):
            for n in (1, 2, 3, 4, 5, 1023, 4 * 262144 + 3, 4 * 8192 * 256 + 5):
                x = rng.uniform(-30, 30, n).astype(F32)
                x[:min(n, 4)] = np.array([30, -30, 0, -0.5], F32)[:min(n, 4)]
                dy = rng.standard_normal(n).astype(F32)
                X, DY, Y, DX = hp.from_numpy(x), hp.from_numpy(dy), hp.full((n,), np.nan, F32), hp.full((n,), np.nan, F32)
                L.call("pdn_gated_sigmoid_fwd_f32", X._ptr, Y._ptr, alpha, n, hp.stream())
                L.call("pdn_gated_sigmoid_bwd_f32", X._ptr, DY._ptr, DX._ptr, alpha, n, hp.stream())
                y_ref, slope = ref.gated_sigmoid(x, float(F32(alpha)))
                assert np.isfinite(Y.get()).all() and np.isfinite(DX.get()).all(), (alpha, n)
                _close(Y.get(), y_ref, RT, AT, (alpha, n, "y"))
                _close(DX.get(), dy * slope, RT, AT, (alpha, n, "dx"))


def check_norm_fallback_paths(dev):
    """The generic-operator fallbacks of CLIPLayerNorm (llm/clip.py:64) and RMSNorm (nn/modules/norm.py:105): a last axis
    that is not a multiple of 4, or above 2048, is outside csrc/rownorm.hip / the rmsnorm kernel and runs as mean / square /
    sqrt / divide nodes on the device.  Forward and backward against float64 at the fused nodes' tolerances; the node types
    show the fused node was not taken.  (nn.LayerNorm has no such fallback: check_reference_layernorm_widths below.)"""
    import pydynet_amd as pdn
    import pydynet_amd.nn as nn
    from pydynet_amd.llm.clip import CLIPLayerNorm
    from pydynet_amd.core.tensor import Graph
    rng = np.random.default_rng(403)
    t = lambda a, g=False: pdn.Tensor(a, dtype=F32, device=dev, requires_grad=g)
    for cols in (6, 50, 130, 2052, 4096):
        rows = (3, 13)
        x = rng.standard_normal(rows + (cols,)).astype(F32)
        w, b = rng.standard_normal(cols).astype(F32), rng.standard_normal(cols).astype(F32)
        dy = rng.standard_normal(rows + (cols,)).astype(F32)
        Graph.clear()
        ln = CLIPLayerNorm((cols,), eps=EPS, dtype=F32).to(dev)
        with ln.scale.device:
            ln.scale.data[...] = ln.scale.xp.asarray(w)
            ln.shift.data[...] = ln.shift.xp.asarray(b)
        X = t(x, True)
        out = ln(X)
        assert type(out).__name__ != "layer_norm", cols
        (out * t(dy)).sum().backward()
        mu, rs = ref.layernorm_stats(x, EPS)
        dx_ref, dw_ref, db_ref = ref.layernorm_bwd(x, w, mu, rs, dy)
        _close(out.numpy(), ref.layernorm_fwd(x, w, b, mu, rs), RT, AT, (cols, "layernorm y"))
        _close(X.grad.get(), dx_ref, 1e-4, 1e-5, (cols, "layernorm dx"))
        _close(ln.scale.grad.get(), dw_ref, 1e-4, 1e-4, (cols, "layernorm dw"))
        _close(ln.shift.grad.get(), db_ref, 1e-4, 1e-4, (cols, "layernorm db"))
        Graph.clear()
        rn = nn.RMSNorm(cols, eps=1e-6, dtype=F32).to(dev)
        with rn.weight.device:
            rn.weight.data[...] = rn.weight.xp.asarray(w)
        X = t(x, True)
        out = rn(X)
        assert type(out).__name__ != "rms_norm", cols
        (out * t(dy)).sum().backward()
        x64, g64 = x.astype(np.float64), dy.astype(np.float64)
        r = np.sqrt(np.square(x64).mean(-1, keepdims=True) + 1e-6)
        z, dz = x64 / r, g64 * w
        _close(out.numpy(), z * w, RT, AT, (cols, "rmsnorm y"))
        _close(X.grad.get(), (dz - z * (z * dz).mean(-1, keepdims=True)) / r, 1e-4, 1e-5, (cols, "rmsnorm dx"))
        _close(rn.weight.grad.get(), (g64 * z).sum((0, 1)), 1e-4, 1e-4, (cols, "rmsnorm dw"))


def check_reference_layernorm_widths(dev):
    """nn.LayerNorm keeps the reference's statistics over the LEADING axes (nn/modules/norm.py:203-218) and, in training on
    float32, is fused.col_norm at EVERY width -- there is no generic fallback for it, which the node type shows.  The same
    five widths therefore reach csrc/fused.hip colnorm_stat_partial / stat_finish / apply / bwd_partial / bwd_finish /
    bwd_apply: a width that is not a multiple of 4, a partial CN_COLS = 32 column tile (6, 50, 130, 2052), more than 2048
    columns, and 300 rows = one full 256-row chunk plus a partial one (the pairwise merge of chunk statistics).  Forward,
    the running statistics, and backward() (dx, dscale, dshift) against a float64 leading-axes statement."""
    import pydynet_amd as pdn
    import pydynet_amd.nn as nn
    from pydynet_amd.core.tensor import Graph
    rng = np.random.default_rng(404)
    t = lambda a, g=False: pdn.Tensor(a, dtype=F32, device=dev, requires_grad=g)
    eps, mom = 1e-6, 0.1
    for cols in (6, 50, 130, 2052, 4096):
        lead = (3, 100)
        x = rng.standard_normal(lead + (cols,)).astype(F32)
        w, b = rng.standard_normal(cols).astype(F32), rng.standard_normal(cols).astype(F32)
        rm0, rv0 = rng.standard_normal(cols).astype(F32), (0.5 + rng.random(cols)).astype(F32)
        dy = rng.standard_normal(lead + (cols,)).astype(F32)
        Graph.clear()
        ln = nn.LayerNorm((cols,), eps=eps, momentum=mom, dtype=F32).to(dev)
        with ln.scale.device:
            for p_, v in ((ln.scale, w), (ln.shift, b), (ln.running_mean, rm0), (ln.running_var, rv0)):
                p_.data[...] = p_.xp.asarray(v)
        X = t(x, True)
        out = ln(X)
        assert type(out).__name__ == "col_norm", (cols, type(out).__name__)
        (out * t(dy)).sum().backward()
        x64, g64, rows = x.astype(np.float64), dy.astype(np.float64), lead[0] * lead[1]
        mu = x64.mean((0, 1))
        var = np.square(x64 - mu).mean((0, 1))
        rs = 1 / np.sqrt(var + eps)
        xh = (x64 - mu) * rs
        db_ref, dw_ref = g64.sum((0, 1)), (g64 * xh).sum((0, 1))
        # tolerances: the last-axis node's (test_rmsnorm_fwd_bwd); running statistics as test_colnorm_forward_backward_large_offset
        _close(out.numpy(), xh * w + b, RT, AT, (cols, "y"))
        _close(ln.running_mean.data.get(), rm0 * (1 - mom) + mom * mu, 1e-5, 1e-6, (cols, "running mean"))
        _close(ln.running_var.data.get(), rv0 * (1 - mom) + mom * var, 2e-4, 0.0, (cols, "running var"))
        _close(X.grad.get(), w * rs * (g64 - db_ref / rows - xh * (dw_ref / rows)), 1e-4, 1e-5, (cols, "dx"))
        _close(ln.scale.grad.get(), dw_ref, 1e-4, 1e-4, (cols, "dscale"))
        _close(ln.shift.grad.get(), db_ref, 1e-4, 1e-4, (cols, "dshift"))


# =====================================================================================================================
# 5. float64 on the device
# =====================================================================================================================
GEMM64 = [(1, 1, 1), (5, 3, 4), (33, 31, 5), (32, 32, 7), (70, 130, 1000), (128, 96, 64), (2, 300, 3), (64, 64, 0)]


def _within(got, want, bound, what):
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    excess = np.abs(got.astype(np.longdouble) - want) - bound
    assert np.all(excess <= 0), (what, "worst excess", float(excess.max()), "bound there", float(bound.reshape(-1)[int(np.argmax(excess))]))


def check_gemm_f64(dev):
    """csrc/gemm64.hip gemm_f64_mfma_kernel: more than one 32 x 32 tile and more than one wave (M or N > 32), all four
    accumulator registers of both 16-row halves, K % 4 != 0 at K = 5 / 7 / 3 (the zero-filled last k step), K = 0,
    alpha != 1, beta != 0 onto a non-zero C and beta = 0 onto NaN (C must not be read), transposed strides, two batch
    dims with a broadcast operand, a row-padded output.  Reference in np.longdouble; the bound is the a-priori one of a
    length-K inner product, (K + 2) u (|alpha| |A| |B| + |beta| |C0|), which a wrong element misses by ~15 orders."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(501)
    with device:
        for M, N, K in GEMM64:
            a, b, c0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
            A, B = hp.from_numpy(a), hp.from_numpy(b)
            got = hp.matmul(A, B).get()
            _within(got, *ref.gemm_longdouble(a, b, c0, 1.0, 0.0), (M, N, K, "matmul"))
            At, Bt = hp.from_numpy(np.ascontiguousarray(a.T)).T, hp.from_numpy(np.ascontiguousarray(b.T)).T
            assert At.shape == (M, K) and At._strides == (1, M) and Bt._strides == (1, K)   # column-major views
            for alpha in (1.0, 0.5):
                for beta in (0.0, 1.0, -0.25):
                    for X, Y, form in ((A, B, "nn"), (At, Bt, "tt"), (A, Bt, "nt")):
                        C = hp.from_numpy(c0 if beta != 0 else np.full((M, N), np.nan))
                        hp.gemm(X, Y, C, alpha=alpha, beta=beta)
                        got = C.get()
                        assert np.isfinite(got).all(), (M, N, K, alpha, beta, form)
                        _within(got, *ref.gemm_longdouble(a, b, c0, alpha, beta), (M, N, K, alpha, beta, form))
                        if K == 0:
                            assert np.array_equal(got, beta * c0 if beta != 0 else np.zeros((M, N))), (alpha, beta)
            # a row-padded output (ldc = N + 3): the columns beyond N keep their values
            big = rng.standard_normal((M, N + 3))
            Cb = hp.from_numpy(big)
            hp.gemm(A, B, Cb[:, :N], alpha=0.5, beta=-0.25)
            got = Cb.get()
            _within(np.ascontiguousarray(got[:, :N]), *ref.gemm_longdouble(a, b, big[:, :N], 0.5, -0.25), (M, N, K, "ldc"))
            assert np.array_equal(got[:, N:], big[:, N:]), (M, N, K, "padding columns")
        # both batch dims, B broadcast over the first and A over the second
        for M, N, K in ((33, 31, 5), (70, 40, 130)):
            a, b = rng.standard_normal((2, 1, M, K)), rng.standard_normal((3, K, N))
            c0 = rng.standard_normal((2, 3, M, N))
            got = hp.matmul(hp.from_numpy(a), hp.from_numpy(b)).get()
            _within(got, *ref.gemm_longdouble(a, b, c0, 1.0, 0.0), (M, N, K, "batched matmul"))
            a2 = rng.standard_normal((2, 3, M, K))
            C = hp.from_numpy(c0)
            hp.gemm(hp.from_numpy(a2), hp.from_numpy(b), C, alpha=0.5, beta=1.0)
            _within(C.get(), *ref.gemm_longdouble(a2, b, c0, 0.5, 1.0), (M, N, K, "batched gemm"))


def check_float64_through_the_tape(dev):
    """A script that never says float32: float64 `@` with backward() (both products of matmul.grad_fn on pdn_gemm_f64), and
    three SGD steps of a default-dtype Linear -> tanh -> Linear with MSE -- float64 GEMM, elementwise, unary and reduce
    kernels -- against the same arithmetic in float64 NumPy at rtol 1e-10; float64 throughout."""
    import pydynet_amd as pdn
    import pydynet_amd.nn as nn
    import pydynet_amd.nn.functional as F
    import pydynet_amd.optim as optim
    from pydynet_amd.core.tensor import Graph
    rng = np.random.default_rng(502)
    Graph.clear()
    a, b, w = rng.standard_normal((70, 130)), rng.standard_normal((130, 50)), rng.standard_normal((70, 50))
    A = pdn.Tensor(a, device=dev, requires_grad=True)
    B = pdn.Tensor(b, device=dev, requires_grad=True)
    out = pdn.matmul(A, B)
    assert A.dtype == np.float64 and out.dtype == np.float64
    (out * pdn.Tensor(w, device=dev)).sum().backward()
    z = np.zeros((1, 1))
    _within(out.numpy(), *ref.gemm_longdouble(a, b, z, 1.0, 0.0), "a @ b")
    _within(A.grad.get(), *ref.gemm_longdouble(w, b.T, z, 1.0, 0.0), "d a")
    _within(B.grad.get(), *ref.gemm_longdouble(a.T, w, z, 1.0, 0.0), "d b")
    # the two-layer network
    Graph.clear()
    np.random.seed(5)
    l1, l2 = nn.Linear(130, 50), nn.Linear(50, 7)
    w1, b1, w2, b2 = (np.array(p.data, copy=True) for p in (l1.weight, l1.bias, l2.weight, l2.bias))
    assert w1.dtype == np.float64
    l1, l2 = l1.to(dev), l2.to(dev)
    params = [l1.weight, l1.bias, l2.weight, l2.bias]
    lr, mom = 0.05, 0.5
    opt = optim.SGD(params, lr=lr, momentum=mom, nesterov=True)
    x, y = rng.standard_normal((64, 130)), rng.standard_normal((64, 7))
    X, Y = pdn.Tensor(x, device=dev), pdn.Tensor(y, device=dev)
    host = [w1, b1, w2, b2]
    vel = [np.zeros_like(p) for p in host]
    for step in range(3):
        opt.zero_grad()
        h = F.tanh(l1(X))
        pred = l2(h)
        loss = F.mse_loss(pred, Y)
        assert h.dtype == pred.dtype == loss.dtype == np.float64, step
        loss.backward()
        opt.step()
        # the same code in NumPy (nn/modules/linear.py, functional.mse_loss, optim.SGD with its nesterov default)
        hh = np.tanh(x @ host[0] + host[1])
        pp = hh @ host[2] + host[3]
        ll = np.square(pp - y).mean()
        dp = 2 * (pp - y) / pp.size
        dh = (dp @ host[2].T) * (1 - hh * hh)
        grads = [x.T @ dh, dh.sum(0), hh.T @ dp, dp.sum(0)]
        assert np.allclose(loss.item(), ll, rtol=1e-10, atol=0.0), (step, loss.item(), ll)
        for p, v, g in zip(host, vel, grads):
            v *= mom
            v += lr * g
            p -= v
            p -= lr * g
        for p, r, name in zip(params, host, ("w1", "b1", "w2", "b2")):
            got = p.data.get()
            assert got.dtype == np.float64 and p.grad.dtype == np.float64
            assert np.allclose(got, r, rtol=1e-10, atol=1e-14), (step, name, float(np.abs(got - r).max()))


def check_float64_elementwise_index_walks(dev):
    """csrc/elementwise.hip in float64 over the eligibility edges of test_strided_elementwise_index_walks (float32 there):
    innermost extents 4 / 8 / 12 / 7 / 33 / 63 / 64 / 65, stride-0 and stride-2 operands, bases off the 16-byte grid,
    transposed views, sliced outputs, in-place forms, divisors around powers of two.  IEEE operations bit-equal to NumPy;
    exp / log / sqrt / sigmoid / tanh at rtol 1e-12; casts and the masked fill bit-exact."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(503)

    def both(shape):
        a = rng.standard_normal(shape)
        return a, hp.from_numpy(a)
    with device:
        x, X = both((3, 17, 6, 24, 2))
        c, C = both((17, 1, 24))
        for k in (0, 1):                                                      # a stride-2 view times a broadcast table
            assert np.array_equal((X[..., k] * C).get(), x[..., k] * c)
            assert np.array_equal((X[..., k] * C - X[..., 1 - k]).get(), x[..., k] * c - x[..., 1 - k])
        for inner in (4, 8, 12, 7, 33, 64, 65, 63):
            a, A = both((5, 3, inner))
            b, B = both((3, 1))
            v, V = both((inner,))
            at, At = a.transpose(1, 0, 2), A.transpose(1, 0, 2)
            assert (A + B).dtype == np.float64
            assert np.array_equal((A + B).get(), a + b)                       # stride-0 innermost operand
            assert np.array_equal((A * V).get(), a * v)                       # row broadcast
            assert np.array_equal((A / B).get(), a / b)
            assert np.array_equal((At - 2.0).get(), at - 2.0)
            assert np.array_equal(hp.maximum(At, V).get(), np.maximum(at, v))
            assert np.array_equal((-At).get(), -at) and np.array_equal(abs(At).get(), np.abs(at))
            assert np.array_equal(hp.ascontiguousarray(At).get(), np.ascontiguousarray(at))
            pos, Pos = np.abs(at) + 0.5, abs(At) + 0.5
            assert np.allclose(hp.exp(At).get(), np.exp(at), rtol=1e-12, atol=0.0)
            assert np.allclose(hp.log(Pos).get(), np.log(pos), rtol=1e-12, atol=1e-15)
            assert np.allclose(hp.sqrt(Pos).get(), np.sqrt(pos), rtol=1e-12, atol=0.0)
            # the reference's piecewise sigmoid / tanh end in 1 - q or q - 1 with q in [0.5, 2]: exp, the sum, the quotient
            # each round at a spacing of up to 2^-52 there, so an ABSOLUTE 8 * 2^-53 rides on the rtol (it matters as x -> 0)
            for sc in (1.0, 1e-3):
                assert np.allclose(hp.sigmoid(At * sc).get(), ref.sigmoid(at * sc), rtol=1e-12, atol=8 * U64)
                assert np.allclose(hp.tanh(At * sc).get(), np.tanh(at * sc), rtol=1e-12, atol=8 * U64)
            if inner > 4:                                                       # operand bases off the 16-byte grid
                assert np.array_equal((A[..., 1:] + A[..., :-1]).get(), a[..., 1:] + a[..., :-1])
                assert np.array_equal((A[:, :, 1:inner - 3] * 3.0).get(), a[:, :, 1:inner - 3] * 3.0)
            O = hp.zeros((5, 3, inner + 4), np.float64)                         # a sliced (row-padded) output
            O[..., :inner] = A * 1.0
            want = np.zeros((5, 3, inner + 4)); want[..., :inner] = a
            assert np.array_equal(O.get(), want)
            A2 = hp.from_numpy(a.copy()); A2 += B; A2 *= V                      # in place
            assert np.array_equal(A2.get(), (a + b) * v)
            # casts (strided source) and the masked fill
            big = at * 1000.0
            Big = At * 1000.0
            assert np.array_equal(Big.astype(np.float32).get(), big.astype(np.float32))
            assert np.array_equal(Big.astype(np.int64).get(), big.astype(np.int64))
            i64 = rng.integers(-2 ** 40, 2 ** 40, (3, 5, inner))
            assert np.array_equal(hp.from_numpy(i64).astype(np.float64).get(), i64.astype(np.float64))
            f32 = (at * np.where(rng.random(at.shape) < 0.1, 1e-6, 30.0)).astype(np.float32)   # some half subnormals
            F_ = hp.from_numpy(f32)
            assert np.array_equal(F_.astype(np.float64).get(), f32.astype(np.float64))
            h16 = F_.astype(np.float16)
            assert np.array_equal(h16.get(), f32.astype(np.float16))
            assert np.array_equal(h16.astype(np.float32).get(), f32.astype(np.float16).astype(np.float32))
            m = a > 0.3
            A3 = hp.from_numpy(a.copy()); A3[hp.from_numpy(m)] = -1.5
            want = a.copy(); want[m] = -1.5
            assert np.array_equal(A3.get(), want)
        y, Y = both((4, 16, 6, 48))
        assert np.array_equal(hp.ascontiguousarray(Y.transpose(0, 2, 1, 3)).get(), np.ascontiguousarray(y.transpose(0, 2, 1, 3)))
        assert np.array_equal(hp.ascontiguousarray(Y.transpose(0, 2, 3, 1)).get(), np.ascontiguousarray(y.transpose(0, 2, 3, 1)))
        for ext in (2, 3, 255, 256, 257, 1023, 1025):                           # divisors around powers of two
            a, A = both((3, ext, 8))
            assert np.array_equal((A.transpose(1, 0, 2) + 1.0).get(), a.transpose(1, 0, 2) + 1.0)
            assert np.array_equal((A.transpose(2, 1, 0) + 1.0).get(), a.transpose(2, 1, 0) + 1.0)


def check_float64_reductions(dev):
    """csrc/reduce.hip in float64 at the shapes of test_reductions (float32 there): innermost / leading / middle / mixed
    axes, the full reduction of 300,000 elements and the 70,000-long vector (multi-stage), a 5000-row column reduction.
    sum / mean within n u sum|x| over the reduced extent n (any summation order); max / min / argmax / argmin exact."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(504)
    with device:
        for shape, axis, keep in (((7, 288), -1, True), ((4, 6, 256), (0, 1), False), ((300, 1000), None, False),
                                  ((5000, 33), 0, False), ((3, 4, 5), 1, True), ((2, 3, 4, 5), (1, 3), False),
                                  ((70000,), 0, False)):
            a = rng.standard_normal(shape)
            A = hp.from_numpy(a)
            n = a.size // np.abs(a).sum(axis=axis, keepdims=keep).size
            bound = n * U64 * np.abs(a).sum(axis=axis, keepdims=keep)
            al = a.astype(np.longdouble)
            for name, scale in (("sum", 1.0), ("mean", 1.0 / n)):
                got = getattr(A, name)(axis, keep).get()
                want = getattr(al, name)(axis=axis, keepdims=keep)
                assert got.dtype == np.float64 and got.shape == want.shape, (shape, axis, name)
                assert np.all(np.abs(got - want) <= bound * scale), (shape, axis, name, float(np.abs(got - want).max()))
            for name in ("max", "min"):
                assert np.array_equal(getattr(A, name)(axis, keep).get(), getattr(a, name)(axis=axis, keepdims=keep)), (shape, name)
            if axis is None or isinstance(axis, int):
                assert np.array_equal(A.argmax(axis).get(), a.argmax(axis)), shape
                assert np.array_equal(A.argmin(axis).get(), a.argmin(axis)), shape


for _fn in (check_pool2d_shape_sweep, check_pool2d_grid_caps, check_im2col_col2im_shape_sweep,
            check_im2col_col2im_large_and_refusals, check_pool_and_conv_through_the_tape,
            check_rnn_cell_kernels, check_lstm_cell_kernels, check_lstm_rnn_modules_against_float64_unroll,
            check_gru_sequence_against_float64_unroll,
            check_layernorm_kernels, check_gated_sigmoid_kernels, check_norm_fallback_paths,
            check_reference_layernorm_widths,
            check_gemm_f64, check_float64_through_the_tape, check_float64_elementwise_index_walks,
            check_float64_reductions):
    device_variants(globals(), _fn)
