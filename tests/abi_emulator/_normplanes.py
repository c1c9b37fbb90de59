"""The block norms' outputs never written (csrc/normplanes.hip, csrc/gemm_rowres.hip): the entries of include/pdn_normplanes.h
(prefix pdnp_) as compositions of emulated launches of the core header -- the projections of `pdn_*_norm_fwd_f32` with the
normalised rows in a scratch array that is dropped, and the packed weight gradient as xn = x * (1 / rms) * w formed here and
contracted against every column block.  The core header's registry is closed to them, so this part carries its own:
`NormPlanesMixin`, its `NOT_EMULATED`, and `extend()`, which makes the installed `EmulatedLib` answer them too.
tests/test_normplanes_abi_cpu.py holds header, exports and this part equal.  The host emulation has no plane pass: the launch
count stays 0.  (TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd import _lib
from . import EmulatedLib
from ._base import view

NOT_EMULATED = ()


def _round256(n):
    return (n + 255) & ~255


class NormPlanesMixin:
    MIN_ROWS = 16384                     # RTS_MIN_ROWS: from where the split-fp16 projection kernel runs (tests lower it)

    def pdnp_gateup_swiglu_norm_supported(self, M, F, K):
        return int(bool(self.pdn_gateup_swiglu_norm_supported(M, F, K)) and M >= self.MIN_ROWS)

    def pdnp_gateup_swiglu_norm_fwd_f32(self, x, norm_w, eps, rms, wg, w_stride, gu, h, M, F, K, ldx, stream):
        if M == 0 or F == 0:
            return 0
        if not (x and norm_w and rms and wg and gu and h):
            return -1
        if not self.pdnp_gateup_swiglu_norm_supported(M, F, K):
            return -2
        xn = np.empty((M, K), np.float32)
        return self.pdn_gateup_swiglu_norm_fwd_f32(x, norm_w, eps, xn.ctypes.data, rms, wg, w_stride, gu, h, M, F, K, ldx, stream)

    def pdnp_qkv_rope_norm_supported(self, M, D, K, L, hd):
        return int(bool(self.pdn_qkv_rope_norm_supported(M, D, K, L, hd)) and M >= self.MIN_ROWS and hd % 4 == 0)

    def pdnp_qkv_rope_norm_fwd_f32(self, x, norm_w, eps, rms, wq, w_stride, qkv, rope, M, D, K, L, hd, ldx, stream):
        if M == 0 or D == 0:
            return 0
        if not (x and norm_w and rms and wq and qkv and rope):
            return -1
        if not self.pdnp_qkv_rope_norm_supported(M, D, K, L, hd):
            return -2
        xn = np.empty((M, K), np.float32)
        return self.pdn_qkv_rope_norm_fwd_f32(x, norm_w, eps, xn.ctypes.data, rms, wq, w_stride, qkv, rope, M, D, K, L, hd, ldx,
                                              stream)

    def pdnp_norm_dw_blocks_supported(self, K, nb_cols, nb):
        return int(K >= 1 and nb >= 1 and nb_cols >= 4 and nb_cols % 4 == 0 and nb_cols * nb < (1 << 24))

    def pdnp_norm_dw_blocks_workspace_bytes(self, K, nb_cols, nb):
        """The library's sizes where no plane route exists: the product's workspace and room for xn."""
        if not self.pdnp_norm_dw_blocks_supported(K, nb_cols, nb):
            return 0
        return _round256(min(self.pdn_gemm_f32_workspace_bytes(288, nb_cols, K, nb), 1 << 28)) + _round256(K * 288 * 4)

    def pdnp_norm_dw_blocks_plane_launches(self, reset):
        return 0

    def pdnp_norm_dw_blocks_f32(self, x, w, rms, G, ldg, dW, dw_stride, beta, K, nb_cols, nb, ws, wsb, stream):
        if not (x and w and rms and G and dW):
            return -1
        if not self.pdnp_norm_dw_blocks_supported(K, nb_cols, nb) or ldg < nb_cols * nb:
            return -2
        if any(int(p or 0) % 16 for p in (x, w, ws)):
            return -1
        if not ws or wsb < _round256(min(self.pdn_gemm_f32_workspace_bytes(288, nb_cols, K, nb), 1 << 28)):
            return -3
        xv = view(x, (K, 288), (288, 1), np.float32)
        inv = np.float32(1) / view(rms, (K,), (1,), np.float32)
        xn = xv * inv[:, None] * view(w, (288,), (1,), np.float32)
        g = view(G, (K, nb * nb_cols), (ldg, 1), np.float32)
        for b in range(nb):
            out = view(int(dW) + 4 * b * dw_stride, (288, nb_cols), (nb_cols, 1), np.float32)
            prod = np.matmul(xn.T, g[:, b * nb_cols:(b + 1) * nb_cols])
            out[...] = prod + np.float32(beta) * out if beta != 0 else prod
        return 0


class NormPlanesEmulatedLib(NormPlanesMixin, EmulatedLib):
    """`EmulatedLib` with the entries of include/pdn_normplanes.h."""


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnp_ entries as well;
    nothing happens on the real library.  The instance goes with the fixture that installed it."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, NormPlanesMixin):
        emu.__class__ = type("NormPlanesOver" + type(emu).__name__, (NormPlanesMixin, type(emu)), {})
        for path in _lib.NORMPLANES_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
