"""The CLIP entry points (csrc/patch_embed.hip): the patch embedding forward / backward with its `supported` query and the
L2 row normalisation, launch counters 24-27.
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from ._base import flat


def _supported(N, C, H, W, p, D):
    return int(N >= 1 and C >= 1 and p >= 4 and p % 4 == 0 and H >= p and W >= p and H % p == 0 and W % p == 0
               and D >= 4 and D % 4 == 0)


def _patches(img, N, C, H, W, p):
    gh, gw = H // p, W // p
    return img.reshape(N, C, gh, p, gw, p).transpose(0, 2, 4, 1, 3, 5).reshape(N * gh * gw, C * p * p)


class ClipMixin:
    def pdn_patch_embed_supported(self, N, C, H, W, p, D):
        return _supported(N, C, H, W, p, D)

    def pdn_patch_embed_fwd_f32(self, img, ker, cls, pos, out, N, C, H, W, p, D, stream):
        if not _supported(N, C, H, W, p, D):
            return -2
        P, K = (H // p) * (W // p), C * p * p
        x = _patches(np.array(flat(img, N * C * H * W).reshape(N, C, H, W)), N, C, H, W, p)
        w = np.array(flat(ker, D * K).reshape(D, K))
        pe = np.array(flat(pos, (P + 1) * D).reshape(P + 1, D))
        o = flat(out, N * (P + 1) * D).reshape(N, P + 1, D)
        o[:, 0] = flat(cls, D) + pe[0]
        o[:, 1:] = (x @ w.T).reshape(N, P, D) + pe[1:]
        self._count(24)
        return 0

    def pdn_patch_embed_bwd_f32(self, img, dout, dker, acc_k, dcls, acc_c, dpos, acc_p, N, C, H, W, p, D, stream):
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
        self._count(25)
        return 0

    def pdn_l2norm_rows_fwd_f32(self, x, y, nrm, rows, cols, stream):
        a = np.array(flat(x, rows * cols).reshape(rows, cols))
        n = np.sqrt(np.square(a).sum(-1, keepdims=True) + np.float32(1e-12))
        flat(nrm, rows)[...] = n[:, 0]
        flat(y, rows * cols).reshape(rows, cols)[...] = a / n
        self._count(26)
        return 0

    def pdn_l2norm_rows_bwd_f32(self, y, nrm, dy, dx, rows, cols, stream):
        yv = np.array(flat(y, rows * cols).reshape(rows, cols))
        g = np.array(flat(dy, rows * cols).reshape(rows, cols))
        n = np.array(flat(nrm, rows))[:, None]
        flat(dx, rows * cols).reshape(rows, cols)[...] = (g - yv * (yv * g).sum(-1, keepdims=True)) / n
        self._count(27)
        return 0
