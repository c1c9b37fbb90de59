"""The RMSNorm backward folded into the layer input gradient (csrc/normgrad.hip): the entries of include/pdn_normgrad.h
(prefix pdng_) as the composition of the two emulated launches of their statement -- the product of
`pdn_gemm_outres_blocks_nt_f32` (formed here at any row count: that entry's gate is a statement about speed) into the
workspace, then `pdn_rmsnorm_bwd_f32` on it.  The core header's registry (`EmulatedLib`, `NOT_EMULATED` in __init__.py) is
closed to them, so this part carries its own: `NormGradMixin`, its `NOT_EMULATED`, and `extend()`, which makes the installed
`EmulatedLib` answer them too.  tests/test_normgrad_abi_cpu.py holds header, exports and this part equal.  The host emulation
has no fused kernel: the launch count stays 0.  (TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import os
import re

import numpy as np

from pydynet_amd import _lib
from . import EmulatedLib
from ._base import view

NOT_EMULATED = ()


def _round16(n):
    return (n + 15) & ~15


def _atoi(text):
    m = re.match(r"\s*[+-]?\d+", text)
    return int(m.group()) if m else 0


def _part_bytes(emu, M):
    """the partial rows of dw: the norm kernel's or the fused kernel's (one per workgroup), whichever is larger"""
    return _round16(max(emu.pdn_rmsnorm_bwd_workspace_bytes(M, 288), min((M + 127) // 128, 256) * 288 * 4))


class NormGradMixin:
    def pdng_outres_blocks_nt_rmsnorm_bwd_supported(self, M, kb, nb):
        return int(M >= 1 and kb > 0 and kb % 32 == 0 and nb >= 1
                   and self.pdn_gemm_outres_supported(M, 288, kb * nb, kb * nb, kb * nb, 288, 1))

    def pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes(self, M, kb, nb):
        """The library's sizes: room for d(xn) only where the shape and the two switches do not let the fused route be expected."""
        if M < 1:
            return 0
        off = lambda name: name in os.environ and _atoi(os.environ[name]) == 0
        fused = (M >= 65536 and kb > 0 and kb % 32 == 0 and 256 <= kb * nb <= 4096
                 and not off("PDN_NORM_BWD_FUSE") and not off("PDN_OUTRES_SPLIT"))
        return _part_bytes(self, M) + (0 if fused else _round16(M * 288 * 4))

    def pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches(self, reset):
        return 0

    def pdng_outres_blocks_nt_rmsnorm_bwd_f32(self, A, W, bstride, kb, nb, x, w, rms, res, dx, dw, acc, M, lda, ws, wsb, stream):
        if M == 0:
            return 0
        if not (A and W and x and w and rms and dx):
            return -1
        if not self.pdng_outres_blocks_nt_rmsnorm_bwd_supported(M, kb, nb) or bstride % 4 or lda % 4 or lda < kb * nb:
            return -2
        if any(int(p or 0) % 16 for p in (x, w, res, dx, ws)):
            return -1
        if not ws or wsb < _part_bytes(self, M):
            return -3
        part = _part_bytes(self, M)
        own = None
        if wsb < part + _round16(M * 288 * 4):                 # (the library takes d(xn) from its allocator then)
            own = np.empty((M, 288), np.float32)
        dxn = own.ctypes.data if own is not None else int(ws) + part
        a = view(A, (M, nb * kb), (lda, 1), np.float32)
        r = np.zeros((M, 288), np.float32)
        for i in range(nb):
            wi = view(int(W) + 4 * i * bstride, (288, kb), (kb, 1), np.float32)
            r += np.matmul(a[:, i * kb:(i + 1) * kb], wi.T)
        view(dxn, (M, 288), (288, 1), np.float32)[...] = r
        self._count(14)                                    # the output-resident product, as the library counts it
        return self.pdn_rmsnorm_bwd_f32(x, w, rms, dxn, res, dx, dw, acc, M, 288, ws, part, stream)


class NormGradEmulatedLib(NormGradMixin, EmulatedLib):
    """`EmulatedLib` with the entries of include/pdn_normgrad.h."""


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdng_ entries as well;
    nothing happens on the real library.  The instance goes with the fixture that installed it."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, NormGradMixin):
        emu.__class__ = type("NormGradOver" + type(emu).__name__, (NormGradMixin, type(emu)), {})
        for path in _lib.NORMGRAD_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
