"""TEST-ONLY NumPy statements of the CLIP entry points of include/pdn_hip.h (csrc/patch_embed.hip), attached to the
emulated library of tests/abi_emulator by the `clip_emulated` fixture below: the patch embedding forward / backward, its
`supported` query, the L2 row normalisation, and launch counters 24-27 next to the emulator's own 24 slots."""
import ctypes

import numpy as np
import pytest

from tests.abi_emulator import flat

SLOTS = 28


def _supported(N, C, H, W, p, D):
    return int(N >= 1 and C >= 1 and p >= 4 and p % 4 == 0 and H >= p and W >= p and H % p == 0 and W % p == 0
               and D >= 4 and D % 4 == 0)


def _patches(img, N, C, H, W, p):
    gh, gw = H // p, W // p
    return img.reshape(N, C, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, C * p * p)


def attach(monkeypatch, emu):
    extra = [0] * (SLOTS - 24)
    base_counters = emu.pdn_kernel_counters

    def count(slot):
        extra[slot - 24] += 1

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out:
            arr = ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))
            for i in range(24, min(int(n), SLOTS)):
                arr[i] = extra[i - 24]
        if reset:
            extra[:] = [0] * len(extra)
        return 0

    def pdn_patch_embed_supported(N, C, H, W, p, D):
        return _supported(N, C, H, W, p, D)

    def pdn_patch_embed_fwd_f32(img, ker, cls, pos, out, N, C, H, W, p, D, stream):
        if not _supported(N, C, H, W, p, D):
            return -2
        P, K = (H // p) * (W // p), C * p * p
        x = _patches(np.array(flat(img, N * C * H * W).reshape(N, C, H, W)), N, C, H, W, p)
        w = np.array(flat(ker, D * K).reshape(D, K))
        pe = np.array(flat(pos, (P + 1) * D).reshape(P + 1, D))
        o = flat(out, N * (P + 1) * D).reshape(N, P + 1, D)
        o[:, 0] = flat(cls, D) + pe[0]
        o[:, 1:] = (x @ w.T).reshape(N, P, D) + pe[1:]
        count(24)
        return 0

    def pdn_patch_embed_bwd_f32(img, dout, dker, acc_k, dcls, acc_c, dpos, acc_p, N, C, H, W, p, D, stream):
        if not _supported(N, C, H, W, p, D):
            return -2
        P, K = (H // p) * (W // p), C * p * p
        g = np.array(flat(dout, N * (P + 1) * D).reshape(N, P + 1, D))
        if dker:
            x = _patches(np.array(flat(img, N * C * H * W).reshape(N, C, H, W)), N, C, H, W, p)
            r = g[:, 1:].reshape(N * P, D).T @ x
            t = flat(dker, D * K)
            t[...] = (t + r.reshape(-1)) if acc_k else r.reshape(-1)
        s = g.sum(0)
        if dpos:
            t = flat(dpos, (P + 1) * D)
            t[...] = (t + s.reshape(-1)) if acc_p else s.reshape(-1)
        if dcls:
            t = flat(dcls, D)
            t[...] = (t + s[0]) if acc_c else s[0]
        count(25)
        return 0

    def pdn_l2norm_rows_fwd_f32(x, y, nrm, rows, cols, stream):
        a = np.array(flat(x, rows * cols).reshape(rows, cols))
        n = np.sqrt(np.square(a).sum(-1, keepdims=True) + np.float32(1e-12))
        flat(nrm, rows)[...] = n[:, 0]
        flat(y, rows * cols).reshape(rows, cols)[...] = a / n
        count(26)
        return 0

    def pdn_l2norm_rows_bwd_f32(y, nrm, dy, dx, rows, cols, stream):
        yv = np.array(flat(y, rows * cols).reshape(rows, cols))
        g = np.array(flat(dy, rows * cols).reshape(rows, cols))
        n = np.array(flat(nrm, rows))[:, None]
        flat(dx, rows * cols).reshape(rows, cols)[...] = (g - yv * (yv * g).sum(-1, keepdims=True)) / n
        count(27)
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def clip_emulated(emulated_hip, monkeypatch):
    """The emulated C ABI (conftest's `emulated_hip`) with the CLIP entry points attached."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield emulated_hip


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading), from whichever library is installed."""
    from pydynet_amd import _lib
    buf = (ctypes.c_int64 * n)()
    _lib.lib().call("pdn_kernel_counters", buf, n, 1)
    return [int(v) for v in buf]
