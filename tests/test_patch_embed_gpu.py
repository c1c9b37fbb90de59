"""The CLIP kernels of csrc/patch_embed.hip against float64 NumPy: the patch embedding forward (patch projection + class
rows + position embedding), its backward (kernel gradient gathered from the image, class / position batch sums), written
into and accumulated onto existing gradient buffers, and the L2 row normalisation.  Shapes: ViT-B/32 (N = 8, 3 x 224 x 224,
p 32, D 768), N = 1 and N = 3, a patch of 16, and a patch of 14 (ViT-L/14) that `pdn_patch_embed_supported` refuses: it
must give the same numbers through the generic nodes.  The launch counters are asserted so a fallback cannot stay green.
Runs on the real MI355X (``-m gpu``) and on the emulated C ABI."""
import ctypes

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core import fused
from pydynet_amd.core.tensor import Graph
from tests.abi_emulator import counters

PE_FWD, PE_BWD, L2_FWD, L2_BWD = 24, 25, 26, 27
SHAPES = [  # N, C, H, W, p, D, taken by the kernels
    (8, 3, 224, 224, 32, 768, True),
    (1, 3, 224, 224, 32, 768, True),
    (3, 3, 96, 64, 32, 128, True),
    (2, 3, 64, 48, 16, 96, True),
    (2, 3, 56, 56, 14, 64, False),
]


def variants(namespace, fn):
    name = fn.__name__.replace("check_", "")

    @pytest.mark.gpu
    def on_gpu(hip):
        Graph.clear()
        fn("hip:0")

    def on_emulator(emulated_hip):
        fn("hip:0")

    namespace[f"test_{name}_gpu"] = on_gpu
    namespace[f"test_{name}_emulated"] = on_emulator


def host(x):
    if isinstance(x, pdn.Tensor):
        return x.numpy()
    return x if isinstance(x, np.ndarray) else x.get()


def close(a, b, what, rt=1e-4):
    a, b = np.asarray(host(a), np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = float(np.abs(a - b).max()), max(float(np.abs(b).max()), 1e-30)
    assert err <= rt * scale, (what, err, scale)


def reference(img, ker, cls, pos, g):
    N, C, H, W = img.shape
    D, _, p, _ = ker.shape
    gh, gw = H // p, W // p
    x = img.astype(np.float64).reshape(N, C, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(N, gh * gw, C * p * p)
    k2 = ker.astype(np.float64).reshape(D, -1)
    out = np.empty((N, gh * gw + 1, D))
    out[:, 0] = cls.reshape(D) + pos[0]
    out[:, 1:] = x @ k2.T + pos[1:]
    g = g.astype(np.float64)
    dker = (g[:, 1:].reshape(-1, D).T @ x.reshape(-1, C * p * p)).reshape(ker.shape)
    dpatch = (g[:, 1:] @ k2).reshape(N, gh, gw, C, p, p)
    dimg = dpatch.transpose(0, 3, 1, 4, 2, 5).reshape(N, C, H, W)
    return out, dker, g[:, 0].sum(0).reshape(cls.shape), g.sum(0), dimg


def check_patch_embed_against_float64(dev):
    rng = np.random.default_rng(0)
    for N, C, H, W, p, D, taken in SHAPES:
        P = (H // p) * (W // p)
        img = rng.standard_normal((N, C, H, W)).astype(np.float32)
        ker = (0.02 * rng.standard_normal((D, C, p, p))).astype(np.float32)
        cls = rng.standard_normal((1, 1, D)).astype(np.float32)
        pos = rng.standard_normal((P + 1, D)).astype(np.float32)
        g = rng.standard_normal((N, P + 1, D)).astype(np.float32)
        out, dker, dcls, dpos, dimg = reference(img, ker, cls, pos, g)
        want_img = N == 3 or not taken                  # the image gradient path on one taken shape and the refused one
        Graph.clear()
        t_img = pdn.Tensor(img, device=dev, requires_grad=want_img)
        t_ker, t_cls, t_pos = (pdn.Tensor(a, device=dev, requires_grad=True) for a in (ker, cls, pos))
        counters()
        y = fused.patch_embed(t_img, t_ker, t_cls, t_pos)
        close(y, out, f"out {N, C, H, W, p, D}")
        (y * pdn.Tensor(g, device=dev)).sum().backward()
        c = counters()
        assert (c[PE_FWD], c[PE_BWD]) == ((1, 1) if taken else (0, 0)), (N, C, H, W, p, D, c[24:])
        close(t_ker.grad, dker, "dkernel")
        close(t_cls.grad, dcls, "dcls")
        close(t_pos.grad, dpos, "dpos")
        if want_img:
            close(t_img.grad, dimg, "dimg")
        # a second pass onto the gradients the leaves now hold: the kernels accumulate into those buffers in place
        y = fused.patch_embed(t_img, t_ker, t_cls, t_pos)
        (y * pdn.Tensor(g, device=dev)).sum().backward()
        close(t_ker.grad, 2 * dker, "dkernel accumulated")
        close(t_cls.grad, 2 * dcls, "dcls accumulated")
        close(t_pos.grad, 2 * dpos, "dpos accumulated")


def check_patch_embed_abi_accumulate_and_nullable(dev):
    from pydynet_amd import hipnp as hp, _lib
    L = _lib.lib()
    rng = np.random.default_rng(1)
    N, C, H, W, p, D = 3, 3, 64, 64, 32, 128
    P, K = (H // p) * (W // p), C * p * p
    assert L.query("pdn_patch_embed_supported", N, C, H, W, p, D) == 1
    assert L.query("pdn_patch_embed_supported", N, C, 56, 56, 14, D) == 0
    assert L.query("pdn_patch_embed_supported", N, C, H, W, p, 130) == 0
    img = rng.standard_normal((N, C, H, W)).astype(np.float32)
    g = rng.standard_normal((N, P + 1, D)).astype(np.float32)
    _, dker, dcls, dpos, _ = reference(img, np.zeros((D, C, p, p), np.float32), np.zeros((1, 1, D), np.float32),
                                       np.zeros((P + 1, D), np.float32), g)
    base_k = rng.standard_normal((D, K)).astype(np.float32)
    base_c = rng.standard_normal((D,)).astype(np.float32)
    base_p = rng.standard_normal((P + 1, D)).astype(np.float32)
    di, dg = hp.asarray(img), hp.asarray(g)
    for acc in (0, 1):
        bk, bc, bp = hp.asarray(base_k), hp.asarray(base_c), hp.asarray(base_p)
        L.call("pdn_patch_embed_bwd_f32", di._ptr, dg._ptr, bk._ptr, acc, bc._ptr, acc, bp._ptr, acc, N, C, H, W, p, D,
               hp.stream())
        close(bk.get(), acc * base_k + dker.reshape(D, K), f"dkernel acc={acc}")
        close(bc.get(), acc * base_c + dcls.reshape(D), f"dcls acc={acc}")
        close(bp.get(), acc * base_p + dpos, f"dpos acc={acc}")
    # only the kernel gradient / only the batch sums
    bk, bp = hp.asarray(base_k), hp.asarray(base_p)
    L.call("pdn_patch_embed_bwd_f32", di._ptr, dg._ptr, bk._ptr, 1, None, 0, None, 0, N, C, H, W, p, D, hp.stream())
    L.call("pdn_patch_embed_bwd_f32", None, dg._ptr, None, 0, None, 0, bp._ptr, 0, N, C, H, W, p, D, hp.stream())
    close(bk.get(), base_k + dker.reshape(D, K), "dkernel alone")
    close(bp.get(), dpos, "dpos alone")
    with pytest.raises(_lib.HipLibraryError) as e:
        L.call("pdn_patch_embed_fwd_f32", di._ptr, bk._ptr, bc._ptr, bp._ptr, bp._ptr, N, C, 56, 56, 14, D, hp.stream())
    assert getattr(e.value, "code", -2) == -2           # PDN_EUNSUPPORTED: nothing launched
    assert counters()[PE_FWD] == 0


def check_l2norm_rows_against_float64(dev):
    from pydynet_amd import hipnp as hp, _lib
    L = _lib.lib()
    rng = np.random.default_rng(2)
    for rows, cols in ((256, 512), (3, 77), (5, 1000)):
        x = rng.standard_normal((rows, cols)).astype(np.float32)
        x[0] *= 1e-3
        dy = rng.standard_normal((rows, cols)).astype(np.float32)
        n = np.sqrt((x.astype(np.float64) ** 2).sum(-1, keepdims=True) + 1e-12)
        y = x / n
        dx = (dy - y * (y * dy).sum(-1, keepdims=True)) / n
        dxa, dya = hp.asarray(x), hp.asarray(dy)
        yo, no, gx = hp.empty((rows, cols), np.float32), hp.empty((rows,), np.float32), hp.empty((rows, cols), np.float32)
        counters()
        L.call("pdn_l2norm_rows_fwd_f32", dxa._ptr, yo._ptr, no._ptr, rows, cols, hp.stream())
        L.call("pdn_l2norm_rows_bwd_f32", yo._ptr, no._ptr, dya._ptr, gx._ptr, rows, cols, hp.stream())
        c = counters()
        assert c[L2_FWD] == 1 and c[L2_BWD] == 1, c[24:]
        close(yo.get(), y, "y", rt=1e-6)
        close(no.get(), n[:, 0], "n", rt=1e-6)
        close(gx.get(), dx, "dx", rt=1e-5)


def test_counter_slots_keep_their_numbers():
    """Asking for the first 24 slots sees exactly those; the CLIP slots follow (include/pdn_hip.h)."""
    from pydynet_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert "Copies min(n, 28)" in text
    for slot, name in ((23, "conv_quad_wgrad_kernel"), (24, "pdn_patch_embed_fwd_f32"), (25, "pdn_patch_embed_bwd_f32"),
                       (26, "pdn_l2norm_rows_fwd_f32"), (27, "pdn_l2norm_rows_bwd_f32")):
        assert f"{slot} {name}" in text, slot


@pytest.mark.gpu
def test_counters_first_24_unchanged_gpu(hip):
    from pydynet_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_int64 * 25)()
    for i in range(25):
        buf[i] = -7
    L.call("pdn_kernel_counters", buf, 24, 1)
    assert buf[24] == -7                                # nothing past n is written


for _f in (check_patch_embed_against_float64, check_patch_embed_abi_accumulate_and_nullable,
           check_l2norm_rows_against_float64):
    variants(globals(), _f)
