"""CLIP's vision-side nodes: patch_embed (patch projection + class token + position embedding) and clip_logits (the
contrastive head).  (One module of `pydynet_amd.core.fused`; the package docstring lists the reference chains each node
replaces.)"""
from __future__ import annotations

import numpy as np

from .. import function as fn
from ..tensor import Tensor, _Operator, concat
from ._common import _hip, _L, _contig, _require_f32, _is_leaf_f32


def patch_project(x, kernel):
    """llm/clip/model.py:17-32 on the generic operators: cut the (N, C, H, W) images into p x p patches and multiply every
    patch, flattened in (c, py, px) order, by the (C p p, D) matrix of the (D, C, p, p) kernel -> (N, P, D)."""
    n, c, h, w = x.shape
    d, pc, ph, pw = kernel.shape
    p = pc * ph * pw
    gh, gw = h // ph, w // pw
    assert c == pc and h % ph == 0 and w % pw == 0
    W = kernel.transpose(1, 2, 3, 0).reshape(p, d)
    x = x.reshape(n, c, gh, ph, gw, pw).transpose(0, 2, 4, 1, 3, 5).reshape(n, gh, gw, p)
    return (x @ W).reshape(n, gh * gw, d)


def _generic_patch_embed(img, kernel, class_emb, pos_emb):
    x = patch_project(img, kernel)
    N, D = x.shape[0], x.shape[-1]
    cls = class_emb.reshape(1, 1, D)
    if N > 1:                          # one class token per image (the reference's concat takes a single image)
        cls = cls + Tensor(np.zeros((N, 1, D), x.dtype), dtype=x.dtype, device=x.device)
    return concat([cls, x], axis=-2) + pos_emb


class patch_embed(_Operator):
    """out (N, P+1, D) = concat([class_emb, patch_project(img, kernel)], -2) + pos_emb, with the class token broadcast over
    the batch (llm/clip/model.py:17-32, 129-130: a 6-D transposed copy, a GEMM, the concat and the add).

    On a HIP device ONE launch (`pdn_patch_embed_fwd_f32`: an fp32-MFMA GEMM gathering its A tile straight from the NCHW
    image, the position row added and the class rows written in the same launch); backward ONE entry point: the kernel
    gradient dOut[:, 1:]^T @ patches (patches gathered from the image again) and the batch sums for the class and position
    embeddings, written straight into the leaves' gradient buffers.  The image gradient, when asked for, is dOut @ kernel
    and a strided copy back to NCHW.  Shapes the kernels do not take (p % 4 != 0, a non-contiguous image, ...) and the
    "cpu" device build the generic composition instead; so does `enabled = False`."""

    enabled = True          # class switch: False builds the generic nodes (tests, A/B)

    @staticmethod
    def applicable(img, kernel, class_emb, pos_emb):
        if not (patch_embed.enabled and isinstance(img, Tensor) and img.device.is_hip and img.ndim == 4 and kernel.ndim == 4):
            return False
        ts = (img, kernel, class_emb, pos_emb)
        if any(t.dtype != np.float32 or t.device != img.device for t in ts):
            return False
        N, C, H, W = img.shape
        D, kc, ph, pw = kernel.shape
        if kc != C or ph != pw or H % ph or W % pw:
            return False
        P = (H // ph) * (W // pw)
        if class_emb.size != D or tuple(pos_emb.shape) != (P + 1, D):
            return False
        if not (img.data.is_contiguous() and img.data._ptr % 16 == 0):
            return False
        return bool(_L().query("pdn_patch_embed_supported", N, C, H, W, ph, D))

    def __new__(cls, img, kernel, class_emb, pos_emb):
        if not isinstance(img, Tensor):
            img = Tensor(np.asarray(img, np.float32), dtype=np.float32, device=kernel.device)
        if cls.applicable(img, kernel, class_emb, pos_emb):
            return object.__new__(cls)
        return _generic_patch_embed(img, kernel, class_emb, pos_emb)

    def __init__(self, img, kernel, class_emb, pos_emb):
        if not isinstance(img, Tensor):
            img = Tensor(np.asarray(img, np.float32), dtype=np.float32, device=kernel.device)
        super().__init__(img, kernel, class_emb, pos_emb)

    def forward_(self, img, kernel, class_emb, pos_emb):
        _require_f32(self, img, kernel, class_emb, pos_emb)
        hp, L = _hip(), _L()
        N, C, H, W = img.shape
        D, p = kernel.shape[0], kernel.shape[2]
        self._geom = (N, C, H, W, p, D)
        self._img = img.data
        self._ker = _contig(kernel.data)
        out = hp.empty((N, pos_emb.shape[0], D), np.float32)
        L.call("pdn_patch_embed_fwd_f32", self._img._ptr, self._ker._ptr, _contig(class_emb.data)._ptr,
               _contig(pos_emb.data)._ptr, out._ptr, N, C, H, W, p, D, hp.stream())
        return out

    def backward_all(self, g):
        img, kernel, cls, pos = self.last
        hp, L = _hip(), _L()
        N, C, H, W, p, D = self._geom
        g = _contig(g)

        def target(t):
            """(buffer, accumulate, returned): the leaf's own gradient buffer when it has one, else a fresh array"""
            if not t.requires_grad:
                return None, 0, None
            if _is_leaf_f32(t):
                return t.grad, 1, None
            buf = hp.empty(t.shape, np.float32)
            return buf, 0, buf
        dk, ak, rk = target(kernel)
        dc, ac, rc = target(cls)
        dp, ap, rp = target(pos)
        if dk is not None or dc is not None or dp is not None:
            L.call("pdn_patch_embed_bwd_f32", self._img._ptr, g._ptr, dk._ptr if dk is not None else None, ak,
                   dc._ptr if dc is not None else None, ac, dp._ptr if dp is not None else None, ap,
                   N, C, H, W, p, D, hp.stream())
        dimg = None
        if img.requires_grad:
            gh, gw = H // p, W // p
            dpatch = hp.matmul(g[:, 1:], self._ker.reshape(D, C * p * p))             # (N, P, C p p)
            dimg = hp.ascontiguousarray(dpatch.reshape(N, gh, gw, C, p, p).transpose(0, 3, 1, 4, 2, 5)).reshape(N, C, H, W)
        return [dimg, rk, rc, rp]


def _generic_clip_logits(img, txt, scale):
    """llm/clip/model.py:195-205 as written there: two L2 normalisations, a transpose, a scale and a product."""
    ni = fn.sqrt(fn.square(img).sum(1, keepdims=True) + 1e-12)
    nt = fn.sqrt(fn.square(txt).sum(1, keepdims=True) + 1e-12)
    return scale * (img / ni) @ (txt / nt).T


class clip_logits(_Operator):
    """logits (B, K) = scale * normalize(img) @ normalize(txt)^T, normalize(x) = x / sqrt(sum(x^2, 1) + 1e-12)
    (llm/clip/model.py:195-205: about 14 generic nodes).

    On a HIP device: `pdn_l2norm_rows_fwd_f32` for each side and ONE GEMM with a Python-number scale folded into its
    alpha; a Tensor scale (one element, as the reference's load_model sets it) multiplies the product on the device --
    no host read -- and receives sum(g * product) when it requires a gradient.  Backward: two GEMMs for the normalised
    features' gradients and `pdn_l2norm_rows_bwd_f32` on each side.  `enabled = False` (and "cpu") builds the generic
    nodes."""

    enabled = True          # class switch: False builds the generic nodes (tests, A/B)

    @staticmethod
    def applicable(img, txt, scale):
        if not (clip_logits.enabled and img.device.is_hip and img.ndim == 2 and txt.ndim == 2
                and img.shape[1] == txt.shape[1] and txt.device == img.device
                and img.dtype == np.float32 and txt.dtype == np.float32):
            return False
        if isinstance(scale, Tensor):
            return scale.size == 1 and scale.dtype == np.float32 and scale.device == img.device
        return isinstance(scale, (int, float, np.integer, np.floating))

    def __new__(cls, img, txt, scale=1.0):
        if cls.applicable(img, txt, scale):
            return object.__new__(cls)
        return _generic_clip_logits(img, txt, scale)

    def __init__(self, img, txt, scale=1.0):
        self._tscale = isinstance(scale, Tensor)
        self.alpha = 1.0 if self._tscale else float(scale)
        super().__init__(*((img, txt, scale) if self._tscale else (img, txt)))

    def _l2(self, x):
        hp, L = _hip(), _L()
        x = _contig(x)
        y, n = hp.empty(x.shape, np.float32), hp.empty((x.shape[0],), np.float32)
        L.call("pdn_l2norm_rows_fwd_f32", x._ptr, y._ptr, n._ptr, x.shape[0], x.shape[1], hp.stream())
        return y, n

    def _l2_bwd(self, y, n, dy):
        hp, L = _hip(), _L()
        dx = hp.empty(y.shape, np.float32)
        L.call("pdn_l2norm_rows_bwd_f32", y._ptr, n._ptr, dy._ptr, dx._ptr, y.shape[0], y.shape[1], hp.stream())
        return dx

    def forward_(self, img, txt, scale=None):
        _require_f32(self, img, txt, scale)
        hp = _hip()
        (self._yi, self._ni), (self._yt, self._nt) = self._l2(img.data), self._l2(txt.data)
        s = hp.empty((img.shape[0], txt.shape[0]), np.float32)
        hp.gemm(self._yi, self._yt.T, s, alpha=self.alpha)
        if not self._tscale:
            return s
        self._s = s
        return s * scale.data.reshape(1, 1)

    def backward_all(self, g):
        hp = _hip()
        img, txt = self.last[0], self.last[1]
        g = _contig(g)
        grads = [None, None]
        if self._tscale:
            scale = self.last[2]
            grads.append((g * self._s).sum().reshape(scale.shape) if scale.requires_grad else None)
            g = g * scale.data.reshape(1, 1)
        if img.requires_grad:
            dyi = hp.empty(self._yi.shape, np.float32)
            hp.gemm(g, self._yt, dyi, alpha=self.alpha)
            grads[0] = self._l2_bwd(self._yi, self._ni, dyi)
        if txt.requires_grad:
            dyt = hp.empty(self._yt.shape, np.float32)
            hp.gemm(g.T, self._yi, dyt, alpha=self.alpha)
            grads[1] = self._l2_bwd(self._yt, self._nt, dyt)
        return grads
