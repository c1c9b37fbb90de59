"""csrc/conv_direct.hip and csrc/conv_quad.hip at every dispatch variant, and at batches larger than the grid.

bench.py's LeNet runs at batch 256 and 4096, where every conv kernel is PERSISTENT over images: a workgroup walks
n, n + gridDim.x, ..., holds the next image in registers (or in the other LDS buffer) while the current one is
multiplied, and a weight-gradient workgroup sums `per_block` images.  The older conv tests stop at 7 images, one per
workgroup.  Here:
  * LARGE: batches of 1027 / 2051 images, compared bit-exactly image by image.  Inputs are small integers (x in
    {-2..2}; w, bias, upstream gradient in {-1, 0, 1}), so every product and partial sum is an integer of magnitude
    <= 2 * N * OH * OW <= 2 * 2051 * 1024 < 2^24: fp32 is exact in any summation order and the float64 reference is
    matched with np.array_equal.  (The emulated ABI has no grid: its variants use 9 images.)
  * VARIANTS: 3 images at shapes chosen, by the launch rules restated in tests/conv_ref.py, to reach every template
    form of the forward / data-gradient kernel and of both weight-gradient kernels, once with standard-normal inputs
    at this suite's direct-conv bound (err <= 2e-5 * max|ref| + 1e-7, tests/test_conv_direct_gpu.py) and once with
    the integer inputs, bit-exact.  A direction the shape's mask refuses must fail with PDN_EUNSUPPORTED and leave
    its output untouched.
  * TAPE: F.conv2d and the conv -> relu -> max_pool chain at shapes whose mask is partial, where one tape node mixes
    direct kernels with the im2col + GEMM / GEMM + col2im route (and the fused node expands its hit map to fall back).
  * the supported-shape masks of the library against the rules the emulator states.
A CPU test asserts that the lists cover the forms named above and that every large batch exceeds its grid."""
import itertools

import numpy as np
import pytest

from tests import conv_ref as R
from tests.conftest import device_variants

UNSUPPORTED = -2                                     # PDN_EUNSUPPORTED (include/pdn_hip.h)
SENTINEL = -12345.0

# (C, H, W, O, k, stride, pad), direct mask (None: only bit 4 is asserted), flags.
# Comments: forward <OT, CH, KS, NV> | weight gradient (lean <KT, OTN, NVD> or regular <WT, PS> +/- register prefetch),
# as tests/conv_ref.py's statements of launch_direct / launch_wgrad select them (PDN_CONV_DEBUG=1 makes the library
# print the weight-gradient choice, to compare).
VARIANTS = [
    ((16, 24, 24, 24, 3, 1, 1), 7, ()),       # (1,4) KS3 NV16 | regular WT2 PS0 (T = 5), no prefetch (C*H*W > 8192), MB 512 of M 576
    ((3, 16, 16, 8, 3, 1, 1), 7, ()),         # (1,2) KS3 NV4 | lean KT1 OTN1 NVD8
    ((6, 8, 8, 40, 3, 1, 1), 7, ()),          # (2,1) KS3 NV4 | lean KT2 OTN2
    ((6, 16, 16, 40, 5, 1, 2), 5, ()),        # (2,2) k = 5 on two tiles: generic KS0 | lean KT5 OTN2, MB halved 256 -> 128
    ((8, 24, 24, 16, 1, 1, 0), 7, ()),        # (1,4) KS1 | lean KT1 OTN1 NVD16 (kern16), MB = M = 576
    ((5, 12, 16, 33, 3, 1, 2), 7, ()),        # (2,2) KS3 NV4, odd C (Cp padding), pad 2 | regular WT1 PS0 (T = 4), prefetch, M = 252 ragged
    ((3, 9, 9, 4, 7, 1, 3), 7, ()),           # (1,1) KS0, k = 7 | regular WT2 PS0 (T = 5)
    ((4, 10, 10, 6, 2, 1, 0), 7, ()),         # (1,1) KS0, k = 2 | regular WT1 PS1
    ((3, 11, 11, 5, 4, 1, 1), 7, ()),         # (1,1) KS0, k = 4: even taps through the data gradient's k-1-pad | regular WT2 PS1
    ((4, 13, 13, 9, 3, 3, 0), 5, ()),         # (1,1) KS3 NV0, stride 3 | regular WT2 PS1
    ((2, 6, 6, 3, 3, 1, 3), 5, ()),           # pad > k-1: border outputs see only padding | regular WT1 PS1
    ((4, 64, 64, 8, 3, 1, 1), 7, ()),         # (1,4) KS3 NV16, in_elems = 16384 exactly | regular WT2 PS1, M = 4096 in MB = 512 blocks
    ((9, 8, 8, 32, 3, 1, 1), 7, ()),          # (1,1) KS3 NV4, O = 32 exactly | lean KT3 OTN1
    ((12, 8, 8, 64, 3, 1, 1), 7, ("null_db",)),  # (2,1) KS3 NV4, O = 64 exactly | lean KT4 OTN2; + a call with db = NULL
    ((16, 8, 8, 20, 3, 1, 1), 7, ("null_dw",)),  # (1,1) KS3 NV4 | lean KT5 OTN1; + a call with dw = NULL
    ((21, 8, 8, 64, 3, 1, 1), 7, ()),         # (2,1) KS3 NV4 | lean KT6 OTN2 at a non-LeNet image
    ((16, 32, 32, 64, 3, 1, 1), 1, ()),       # (2,2) KS3 NV16; forward only
    ((30, 8, 8, 64, 3, 1, 1), 3, ()),         # (2,1) KS3 NV4; weight gradient refused (T = 18)
    ((7, 8, 8, 96, 3, 1, 1), 6, ()),          # forward refused (OPAD 96) | regular WT2 PS0 (T = 6), prefetch
    ((12, 8, 8, 65, 3, 1, 1), 6, ()),         # | regular WT3 PS0 (T = 12), prefetch
    ((10, 12, 12, 96, 3, 1, 1), 4, ()),       # | regular WT3 PS0 (T = 9), prefetch
    ((7, 8, 8, 128, 3, 1, 1), 4, ()),         # | regular WT2 PS0 (T = 8)
    ((12, 8, 8, 128, 3, 1, 1), None, ()),     # | regular WT4 PS0 (T = 16)
    # beyond the issue's table
    ((3, 8, 8, 1, 3, 1, 1), 7, ()),           # O = 1 | lean KT1 OTN1
    ((6, 10, 10, 12, 5, 1, 2), 7, ("no_bias",)),  # (1,1) KS5: the unrolled 5x5 taps, bias = NULL | regular WT2 PS0 (T = 5)
    ((8, 24, 24, 12, 3, 1, 1), 7, ()),        # (1,4) KS3 NV8 | lean KT3 OTN1 NVD16
    ((9, 7, 7, 32, 3, 1, 1), 7, ()),          # (1,1) KS3 NV0 | regular WT3 PS1 (T = 3), no prefetch (W % 4)
    ((9, 6, 4, 32, 3, 1, 1), 7, ()),          # (1,1) KS3 NV4 | regular WT3 PS1 (T = 3), prefetch (M = 24 is no multiple of 32)
    ((30, 8, 8, 65, 3, 1, 1), 2, ()),         # data gradient only
    ((65, 6, 6, 70, 3, 1, 1), 0, ()),         # nothing direct
]

# batches past the grid on the plain entries: case, N on the GPU
LARGE_DIRECT = [
    ((4, 8, 8, 8, 3, 1, 1), 2051),            # grid 1024, (1,1) KS3 NV4 register prefetch | lean KT2, 411 workgroups x 5 images
    ((16, 24, 24, 24, 3, 1, 1), 1027),        # grid 512, (1,4) KS3 NV16 | regular, 206 workgroups x 5 images, two position blocks
    ((5, 9, 11, 7, 3, 2, 1), 2051),           # grid 1024, NV0: stage_image; no data gradient (stride 2)
]
LARGE_FUSED = ((4, 8, 8, 8), 2051)            # EP = 1 / SRC = 1 forms of the generic kernels, lean weight gradient with dmask
LARGE_QUAD = [((3, 32, 32, 20), 1027), ((20, 16, 16, 50), 1027)]      # csrc/conv_quad.hip: both LeNet layers
EMULATED_N = 9

TAPE_CONV = [c for c, m, _ in VARIANTS if m in (0, 1, 2, 3, 4, 5, 6)]     # every row whose mask is partial (or empty)
TAPE_CHAIN = [((16, 32, 32, 64), 1), ((16, 32, 32, 16), 3)]           # (C, H, W, O), fused mask (k 3, stride 1, pad 1)


def _emulator_rules():
    from tests.abi_emulator._conv import ConvMixin
    return ConvMixin()


def _batch(n_gpu):
    """EMULATED_N images only where the installed library IS the emulator; anything else runs the batch past the grid."""
    from pydynet_amd import _lib
    from tests.abi_emulator import EmulatedLib
    return EMULATED_N if isinstance(_lib.lib(), EmulatedLib) else n_gpu


def _close(got, ref, what):
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    print(what, "err", err, "scale", scale)
    assert err <= 2e-5 * scale + 1e-7, (what, err, scale)


def _exact(got, ref, what):
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not np.array_equal(got, ref):
        bad = np.flatnonzero((got != ref).reshape(got.shape[0], -1).any(1))
        raise AssertionError((what, "differs in rows (images, where the leading axis is the batch)", bad[:8].tolist(),
                              "of", got.shape[0], "count", int(bad.size)))


def _refused(L, hp, name, outs, *args):
    from pydynet_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError) as e:
        L.call(name, *args)
    assert e.value.code == UNSUPPORTED, (name, e.value.code)
    hp.synchronize()
    for out in outs:
        assert np.all(out.get() == np.float32(SENTINEL)), (name, "wrote to its output although it refused the shape")


def _direct_entries(dev, case, N, integer, want_mask, flags=()):
    """pdn_conv2d_fwd_f32 / _bwd_data_f32 / _bwd_weight_f32 (accumulate 0, then 1) against the float64 reference."""
    import pydynet_amd as pdn  # noqa: F401
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.cuda import Device
    L = _lib.lib()
    C, H, W, O, k, s, p = case
    oh, ow = R.out_hw(H, W, k, s, p)
    rng = np.random.default_rng(sum(case) + N + int(integer))
    x, w, b, g = (R.integer_inputs if integer else R.normal_inputs)(rng, N, C, H, W, O, k, (N, O, oh, ow))
    bias = None if "no_bias" in flags else b
    y_ref, dx_ref, dw_ref, db_ref = R.conv_ref(x, w, bias, g, s, p)
    same = _exact if integer else _close
    tag = (case, N, "integer" if integer else "normal")
    mask = L.query("pdn_conv2d_direct_supported", C, H, W, O, k, s, p)
    if want_mask is None:
        assert mask & 4, (case, mask)
    else:
        assert mask == want_mask, (case, mask, want_mask)
    with Device(dev):
        X, Wd, B, G = (hp.from_numpy(a) for a in (x, w, b, g))
        geom = (N, C, H, W, O, k, s, p)
        Y = hp.full((N, O, oh, ow), SENTINEL, np.float32)
        args = (X._ptr, Wd._ptr, B._ptr if bias is not None else None, Y._ptr) + geom + (hp.stream(),)
        if mask & 1:
            L.call("pdn_conv2d_fwd_f32", *args)
            same(Y.get(), y_ref, tag + ("y",))
        else:
            _refused(L, hp, "pdn_conv2d_fwd_f32", (Y,), *args)
        DX = hp.full((N, C, H, W), SENTINEL, np.float32)
        args = (G._ptr, Wd._ptr, DX._ptr) + geom + (hp.stream(),)
        if mask & 2:
            L.call("pdn_conv2d_bwd_data_f32", *args)
            same(DX.get(), dx_ref, tag + ("dx",))
        else:
            _refused(L, hp, "pdn_conv2d_bwd_data_f32", (DX,), *args)
        DW = hp.full((O, C, k, k), SENTINEL, np.float32)
        DB = hp.full((O,), SENTINEL, np.float32)
        ws, wsb = hp.workspace(L.query("pdn_conv2d_bwd_weight_workspace_bytes", *geom))
        if mask & 4:
            for acc in (0, 1):                           # accumulate = 0 overwrites the sentinel; = 1 adds a second time
                L.call("pdn_conv2d_bwd_weight_f32", X._ptr, G._ptr, DW._ptr, DB._ptr, acc, *geom, ws, wsb, hp.stream())
                same(DW.get(), (acc + 1) * dw_ref, tag + ("dw", "accumulate", acc))
                same(DB.get(), (acc + 1) * db_ref, tag + ("db", "accumulate", acc))
            # further calls with one output NULL: the other one is still right (it overwrites a fresh sentinel)
            for flag, name in (("null_dw", "db"), ("null_db", "dw")):
                if flag in flags:
                    out = hp.full((O,) if name == "db" else (O, C, k, k), SENTINEL, np.float32)
                    dwp, dbp = (None, out._ptr) if name == "db" else (out._ptr, None)
                    L.call("pdn_conv2d_bwd_weight_f32", X._ptr, G._ptr, dwp, dbp, 0, *geom, ws, wsb, hp.stream())
                    same(out.get(), db_ref if name == "db" else dw_ref, tag + (name, "alone: the other output NULL"))
        else:
            _refused(L, hp, "pdn_conv2d_bwd_weight_f32", (DW, DB), X._ptr, G._ptr, DW._ptr, DB._ptr, 0, *geom, ws, wsb,
                     hp.stream())


def _tape(dev, x, w, b, g, s, p, pool, x_grad=True):
    """F.conv2d (then relu and max_pool2d(2, 2) when `pool`) under the upstream gradient g: node type, out, dx, dw, db."""
    import pydynet_amd as pdn
    import pydynet_amd.nn.functional as F
    from pydynet_amd.core.tensor import Graph
    Graph.clear()
    X = pdn.Tensor(x, dtype=np.float32, device=dev, requires_grad=x_grad)
    Wt = pdn.Tensor(w, dtype=np.float32, device=dev, requires_grad=True)
    Bt = pdn.Tensor(b.reshape(1, -1, 1, 1), dtype=np.float32, device=dev, requires_grad=True)
    out = F.conv2d(X, Wt, p, s, Bt)
    if pool:
        out = F.max_pool2d(F.relu(out), 2, 2)
    kind = type(out).__name__
    (out * pdn.Tensor(g, dtype=np.float32, device=dev)).sum().backward()
    got = kind, out.numpy(), (X.grad.get() if x_grad else None), Wt.grad.get(), Bt.grad.get().reshape(-1)
    Graph.clear()
    return got


def _quad_counters(reset=False):
    import ctypes
    from pydynet_amd import _lib
    buf = (ctypes.c_int64 * 24)()
    _lib.lib().call("pdn_kernel_counters", buf, 24, 1 if reset else 0)
    return tuple(int(v) for v in buf[21:24])


def _large_chain(dev, shape, n_gpu, quad):
    """The fused chain at a batch past every grid, with and without a gradient for x: bit-exact, every image."""
    C, H, W, O = shape
    N = _batch(n_gpu)
    rng = np.random.default_rng(N + sum(shape))
    x, w, b, gp = R.integer_inputs(rng, N, C, H, W, O, 3, (N, O, H // 2, W // 2))
    ref = R.conv_relu_pool_ref(x, w, b, gp)
    for x_grad in (True, False):
        _quad_counters(reset=True)
        kind, out, dx, dw, db = _tape(dev, x, w, b, gp, 1, 1, True, x_grad)
        assert kind == "conv2d_relu_pool", (shape, kind)
        # conv1 has no fused data gradient (a network's first layer): asked for dx, its node expands the pooled
        # gradient and runs the plain kernels (tests/test_conv_relu_pool.py expects the same launch counts)
        want = {(3, 32, 32, 20): ((1, 0, 0), (1, 0, 1)), (20, 16, 16, 50): ((1, 1, 1), (1, 0, 1))}[shape] if quad \
            else ((0, 0, 0), (0, 0, 0))
        assert _quad_counters() == want[0 if x_grad else 1], (shape, x_grad, _quad_counters())
        tag = (shape, N, "x_grad", x_grad)
        _exact(out, ref[0], tag + ("pooled",))
        if x_grad:
            _exact(dx, ref[1], tag + ("dx",))
        else:
            assert dx is None
        _exact(dw, ref[2], tag + ("dw",))
        _exact(db, ref[3], tag + ("db",))


def _name(case):
    return "x".join(str(v) for v in case[:3]) + f"_o{case[3]}" + (f"_k{case[4]}s{case[5]}p{case[6]}" if len(case) > 4 else "")


def _register(fn, name):
    fn.__name__ = "check_" + name
    device_variants(globals(), fn)


# ---- 2. batches past the grid ---------------------------------------------------------------------------------------
for _case, _n in LARGE_DIRECT:
    def _check(dev, case=_case, n=_n):
        mask = _emulator_rules().pdn_conv2d_direct_supported(*case)
        _direct_entries(dev, case, _batch(n), True, mask)
    _register(_check, f"large_batch_direct_{_name(_case)}")


def _check(dev):
    _large_chain(dev, LARGE_FUSED[0], LARGE_FUSED[1], quad=False)


_register(_check, f"large_batch_fused_generic_{_name(LARGE_FUSED[0])}")

for _shape, _n in LARGE_QUAD:
    def _check(dev, shape=_shape, n=_n):
        _large_chain(dev, shape, n, quad=True)
    _register(_check, f"large_batch_fused_quad_{_name(_shape)}")


# ---- 3. the dispatch variants at three images -------------------------------------------------------------------------
for _case, _mask, _flags in VARIANTS:
    def _check(dev, case=_case, mask=_mask, flags=_flags):
        for integer in (False, True):
            _direct_entries(dev, case, 3, integer, mask, flags)
    _register(_check, f"variant_{_name(_case)}")


# ---- 4. through the tape at partial masks ------------------------------------------------------------------------------
for _case in TAPE_CONV:
    def _check(dev, case=_case):
        C, H, W, O, k, s, p = case
        oh, ow = R.out_hw(H, W, k, s, p)
        for integer in (False, True):
            rng = np.random.default_rng(sum(case) + int(integer))
            x, w, b, g = (R.integer_inputs if integer else R.normal_inputs)(rng, 3, C, H, W, O, k, (3, O, oh, ow))
            if integer:                                  # "a random upstream gradient": exact all the same as long as
                g = rng.integers(-3, 4, g.shape).astype(np.float32)      # it is a small integer (sums stay far below 2^24)
            ref = R.conv_ref(x, w, b, g, s, p)
            kind, *got = _tape(dev, x, w, b, g, s, p, pool=False)
            assert kind == "conv2d", kind
            for a, r, name in zip(got, ref, ("y", "dx", "dw", "db")):
                (_exact if integer else _close)(a, r, (case, "integer" if integer else "normal", name))
    _register(_check, f"tape_conv2d_{_name(_case)}")

for _shape, _fmask in TAPE_CHAIN:
    def _check(dev, shape=_shape, fmask=_fmask):
        from pydynet_amd import _lib
        C, H, W, O = shape
        assert _lib.lib().query("pdn_conv2d_relu_pool_supported", C, H, W, O, 3, 1, 1) == fmask
        # integer inputs only: ties and exact zeros occur and are decided exactly on both sides (with real-valued inputs a
        # window whose two largest entries differ by an fp32 round-off would make the comparison ill-posed)
        rng = np.random.default_rng(sum(shape))
        x, w, b, gp = R.integer_inputs(rng, 3, C, H, W, O, 3, (3, O, H // 2, W // 2))
        gp = rng.integers(-3, 4, gp.shape).astype(np.float32)
        ref = R.conv_relu_pool_ref(x, w, b, gp)
        kind, *got = _tape(dev, x, w, b, gp, 1, 1, pool=True)
        assert kind == "conv2d_relu_pool", kind
        for a, r, name in zip(got, ref, ("pooled", "dx", "dw", "db")):
            _exact(a, r, (shape, name))
    _register(_check, f"tape_chain_{_name(_shape)}")

del _check, _case, _shape


# ---- 5. the library and the emulator agree on what is supported ------------------------------------------------------------
SUPPORT_GRID = dict(C=(1, 2, 3, 5, 8, 16, 20, 21, 30, 64), HW=(3, 7, 8, 9, 16, 24, 32, 64),
                    O=(1, 31, 32, 33, 64, 65, 96, 128, 129), k=(1, 2, 3, 4, 5, 7), s=(1, 2, 3))


def _support_combinations():
    G = SUPPORT_GRID
    for k in G["k"]:
        for p in sorted({0, 1, 2, 3, k}):
            for C, H, W, O, s in itertools.product(G["C"], G["HW"], G["HW"], G["O"], G["s"]):
                yield C, H, W, O, k, s, p


def _masks_disagree(direct, fused):
    """Combinations of SUPPORT_GRID at which (direct, fused) differ from the emulator's two rules."""
    emu = _emulator_rules()
    bad = []
    for c in _support_combinations():
        got = direct(*c), fused(*c)
        want = emu.pdn_conv2d_direct_supported(*c), emu.pdn_conv2d_relu_pool_supported(*c)
        if got != want:
            bad.append((c, got, want))
    return bad


@pytest.mark.gpu
def test_supported_masks_of_library_equal_emulator_rules(hip):
    """Host queries only, no launch: 466 560 shapes, both masks."""
    from pydynet_amd import _lib
    fn = _lib.lib().fn
    bad = _masks_disagree(fn["pdn_conv2d_direct_supported"], fn["pdn_conv2d_relu_pool_supported"])
    assert not bad, (len(bad), bad[:10])


# ---- coverage of the lists (CPU) -------------------------------------------------------------------------------------------
def test_case_lists_cover_every_dispatch_form_and_exceed_their_grids():
    emu = _emulator_rules()
    fwd, lean, regular, halved = set(), set(), set(), False
    for case, want, _ in VARIANTS + [(c, None, ()) for c, _ in LARGE_DIRECT]:
        mask = emu.pdn_conv2d_direct_supported(*case)
        assert want is None or mask == want, (case, mask, want)
        if mask & 1:
            fwd.add(R.forward_variant(*case, 3)[:4])
        if mask & 2:
            fwd.add(R.dgrad_variant(*case, 3)[:4])
        if mask & 4:
            v = R.wgrad_variant(*case, 3)
            if v[0] == "lean":
                lean.add(v[1:4])
                halved |= v[5]
            else:
                regular.add(v[1:4])
    assert {(ot, ch) for ot, ch, _, _ in fwd} == {(1, 1), (1, 2), (1, 4), (2, 1), (2, 2)}
    assert {ks for _, _, ks, _ in fwd} == {0, 1, 3, 5}
    assert {nv for _, _, _, nv in fwd} == {0, 4, 8, 16}
    # what the older direct tests never reached: NV16 on (1,4), a (1,2) tile, (2,1) and (1,1) on the prefetch path,
    # the generic taps on two output tiles, 1x1 taps on (1,4)
    assert {(1, 4, 3, 16), (1, 2, 3, 4), (2, 1, 3, 4), (1, 1, 3, 4), (2, 2, 0, 0), (1, 4, 1, 0), (2, 2, 3, 16)} <= fwd
    assert {kt for kt, _, _ in lean} == {1, 2, 3, 4, 5, 6}
    assert {otn for _, otn, _ in lean} == {1, 2} and {nvd for _, _, nvd in lean} == {8, 16}
    assert {kt for kt, otn, _ in lean if otn == 2} >= {2, 4, 5, 6} and halved
    assert {(wt, ps) for wt, ps, _ in regular} == {(1, 1), (2, 1), (3, 1), (1, 0), (2, 0), (3, 0), (4, 0)}
    assert {pre for _, _, pre in regular} == {True, False}
    assert {emu.pdn_conv2d_direct_supported(*c) for c in TAPE_CONV} == {0, 1, 2, 3, 4, 5, 6}
    for shape, want in TAPE_CHAIN:
        assert emu.pdn_conv2d_relu_pool_supported(*shape, 3, 1, 1) == want, shape

    # a batch past the grid: some workgroup takes a second image, and the last sweep is ragged (workgroups with no
    # next image); a weight-gradient workgroup sums several images and the last one fewer
    def past(n, grid):
        return n > grid and n % grid != 0
    for case, n in LARGE_DIRECT + [(LARGE_FUSED[0] + (3, 1, 1), LARGE_FUSED[1])]:
        mask = emu.pdn_conv2d_direct_supported(*case)
        assert past(n, R.forward_variant(*case, n)[4]), case
        assert not mask & 2 or past(n, R.dgrad_variant(*case, n)[4]), case
        v = R.wgrad_variant(*case, n)
        assert v[7] >= 2 and n % v[7] != 0 and v[6] * v[7] >= n > (v[6] - 1) * v[7], (case, v)
        oh, ow = R.out_hw(*case[1:3], *case[4:])
        assert 2 * n * oh * ow < 2 ** 24                 # the integer inputs stay exact in fp32
    assert R.forward_variant(*LARGE_DIRECT[0][0], 2051)[:4] == (1, 1, 3, 4)
    assert R.forward_variant(*LARGE_DIRECT[1][0], 1027)[:4] == (1, 4, 3, 16)
    assert R.forward_variant(*LARGE_DIRECT[2][0], 2051)[3] == 0
    for shape, n in LARGE_QUAD:
        f, d, wg, ipt = R.quad_grids(*shape, n)
        groups = (n + ipt - 1) // ipt
        assert groups > 2 * f and groups % f != 0 and n % ipt == (1 if ipt == 2 else 0), shape   # a third, ragged sweep
        assert (n + 3) // 4 > d and n % 4 != 0 and n > 2 * 256 and n % wg != 0, shape
        assert 2 * n * shape[1] * shape[2] < 2 ** 24
    assert EMULATED_N % 2 == 1


def test_chunked_reference_equals_the_one_block_statement():
    """tests/conv_ref.py in blocks of 2 images against its own one-block run and a direct (loop) statement."""
    rng = np.random.default_rng(0)
    N, C, H, W, O, k, s, p = 5, 3, 7, 6, 4, 3, 2, 2
    oh, ow = R.out_hw(H, W, k, s, p)
    x, w, b, g = R.normal_inputs(rng, N, C, H, W, O, k, (N, O, oh, ow))
    one, two = R.conv_ref(x, w, b, g, s, p, block=64), R.conv_ref(x, w, b, g, s, p, block=2)
    xp = np.pad(x.astype(np.float64), [(0, 0), (0, 0), (p, p), (p, p)])
    y = np.zeros((N, O, oh, ow)); dxp = np.zeros_like(xp); dw = np.zeros(w.shape)
    for oy, ox in itertools.product(range(oh), range(ow)):
        patch = xp[:, :, oy * s:oy * s + k, ox * s:ox * s + k]
        y[:, :, oy, ox] = np.einsum("nckl,ockl->no", patch, w.astype(np.float64)) + b
        dw += np.einsum("no,nckl->ockl", g[:, :, oy, ox].astype(np.float64), patch)
        dxp[:, :, oy * s:oy * s + k, ox * s:ox * s + k] += np.einsum("no,ockl->nckl", g[:, :, oy, ox].astype(np.float64), w.astype(np.float64))
    loop = y, dxp[:, :, p:p + H, p:p + W], dw, g.astype(np.float64).sum((0, 2, 3))
    for a, b_, c in zip(one, two, loop):
        assert np.allclose(a, b_, rtol=1e-13, atol=1e-13) and np.allclose(a, c, rtol=1e-12, atol=1e-12)
    # the pooled chain: blocks against one block, on integer inputs (ties, exact zeros)
    x, w, b, gp = R.integer_inputs(rng, 5, 3, 8, 8, 4, 3, (5, 4, 4, 4))
    for a, b_ in zip(R.conv_relu_pool_ref(x, w, b, gp, block=64), R.conv_relu_pool_ref(x, w, b, gp, block=2)):
        assert np.array_equal(a, b_)
