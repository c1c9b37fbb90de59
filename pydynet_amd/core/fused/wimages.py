"""All weight plane images of a pass in one launch (include/pdn_wimages.h, csrc/weight_images.hip).
(One module of `pydynet_amd.core.fused`.)

The split-fp16 products of a Llama layer each turn their weight into fp16 plane images first: thirteen small launches per
layer and step, each directly in front of the product that waits for it.  Nothing changes a weight inside a forward pass or
inside a backward pass, so the model describes the products of a pass up front (`layer_forms`), an `ImageSet` builds all
their images in ONE launch into an arena of its own and binds it for the pass; a product whose weight operand matches a
descriptor takes its image from the set, any other builds its own as before.  Nothing outlives the pass: the weights are
read when the forward pass starts and again when the backward pass starts, exactly the passes in which the per-call
launches read them, so a weight changed between two passes is seen as it always was, and there is nothing to invalidate.
PDN_WIMAGES=0 (read at every pass) keeps the per-call launches."""
from __future__ import annotations

import ctypes
import os

import numpy as np

from ._common import _hip, _L, _provides

min_rows = 65536            # the output-resident split products take 65536 rows and more (csrc/outres_split_index.h)


def enabled():
    hp = _hip()
    return os.environ.get("PDN_WIMAGES", "1") != "0" and _provides("pdnw_set_build") and hp.capturing() is None


class ImageSet:
    """Descriptor constructor calls (entry name, arguments: the weight operands the product's own entry gets) of one pass.
    `bind()` builds the images into a fresh arena in one launch and makes the set the thread's current one; `release()` unbinds
    and lets go of the arena.  `keep`: whatever the descriptors point into."""

    def __init__(self, ctors, keep=()):
        self.ctors, self._keep, self._arena, self._recs = list(ctors), tuple(keep), None, None

    def bind(self):
        if not self.ctors or not enabled():
            return False
        hp, L = _hip(), _L()
        n, nb = len(self.ctors), L.query("pdnw_desc_bytes")
        recs = ctypes.create_string_buffer(nb * n)
        for i, (name, args) in enumerate(self.ctors):
            L.call(name, ctypes.addressof(recs) + i * nb, *args)
        nbytes = L.query("pdnw_set_bytes", recs, n)
        if nbytes <= 0:
            return False
        arena = hp.empty((nbytes // 4,), np.float32)
        L.call("pdnw_set_build", recs, n, arena._ptr, hp.stream())
        L.call("pdnw_bind", recs, n, arena._ptr, hp.stream())
        self._arena, self._recs = arena, recs
        return True

    def release(self):
        _L().call("pdnw_unbind")
        self._arena = self._recs = None


def _f32c(*arrays):
    hp = _hip()
    return all(isinstance(a, hp.ndarray) and a.dtype == np.float32 and a.is_contiguous() and a._ptr % 16 == 0 for a in arrays)


def layer_forms(wq, wk, wv, wo, wg, wu, wd, T, Lq, hd):
    """(forward, backward) descriptor constructor calls for one layer's eight images -- forward: q | k | v, Wo, gate | up,
    down; backward: dX of q | k | v, dz Wo^T, dh, dX of gate | up -- for those products the split routes will take at T rows
    (the existing *_supported queries and switches decide; a product that then runs elsewhere, or with other operands, simply
    does not find its image).  The arguments are the weights' device arrays."""
    L = _L()
    fwd, bwd = [], []
    D = wq.shape[0]
    if T < min_rows or D != 288 or not _f32c(wq, wk, wv, wo, wg, wu, wd):
        return fwd, bwd
    F = wg.shape[1]
    qkv_stride, gu_stride = (wk._ptr - wq._ptr) // 4, (wu._ptr - wg._ptr) // 4
    qkv_packed = wq.shape == wk.shape == wv.shape == (D, D) and wv._ptr - wk._ptr == wk._ptr - wq._ptr and qkv_stride % 4 == 0
    gu_packed = wg.shape == wu.shape and abs(gu_stride) >= D * F and abs(gu_stride) + D * F < (1 << 30) and gu_stride % 4 == 0
    # the projection kernels (csrc/rowtile_split.hip): the queries include the switches of the split form
    if qkv_packed and L.query("pdnp_qkv_rope_norm_supported", T, D, D, Lq, hd):
        fwd.append(("pdnw_desc_qkv", (wq._ptr, qkv_stride, D, D)))
    if gu_packed and L.query("pdnp_gateup_swiglu_norm_supported", T, F, D):
        fwd.append(("pdnw_desc_gateup", (wg._ptr, gu_stride, F, D)))
        if wd.shape == (F, D) and F % 32 == 0:
            bwd.append(("pdnw_desc_down_t", (wd._ptr, F, D)))
    # the output-resident products (csrc/outres_split.hip)
    if os.environ.get("PDN_OUTRES_SPLIT", "1") != "0" and L.query("pdn_gemm_rowtile_mode", -1) != 3:
        if wo.shape == (D, D):
            fwd.append(("pdnw_desc_outres", (wo._ptr, D, D, 0, 0, 0)))
            bwd.append(("pdnw_desc_outres", (wo._ptr, D, D, 1, 0, 0)))
        if wd.shape == (F, D) and F % 32 == 0 and 256 <= F <= 4096:
            fwd.append(("pdnw_desc_outres", (wd._ptr, F, D, 0, 0, 0)))
        if qkv_packed and L.query("pdn_gemm_outres_blocks_supported", T, D, 3):
            bwd.append(("pdnw_desc_outres", (wq._ptr, 3 * D, D, 1, D, qkv_stride)))
        if gu_packed and F % 32 == 0 and 2 * F <= 4096 and L.query("pdn_gemm_outres_blocks_supported", T, F, 2):
            bwd.append(("pdnw_desc_outres", (wg._ptr, 2 * F, F, 1, F, gu_stride)))
    return fwd, bwd
