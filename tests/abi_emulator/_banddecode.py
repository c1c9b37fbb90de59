"""The entries of include/pdn_banddecode.h (prefix pdnv_, csrc/decode_band.hip), answered with their statement: query head h
over key/value head h // G and the keys [max(0, pos - window + 1), pos]; a part with a registry of its own, as
tests/abi_emulator/_gqdecode.py.  Launch counter slot 58 is kept here.  (TEST-ONLY.)"""
import ctypes
import math

import numpy as np

from pydynet_amd import _lib
from . import EmulatedLib
from ._base import flat, view
from ._extend import rotate

NOT_EMULATED = ()
SLOT = 58


class BandDecodeMixin:
    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[SLOT] = self.__dict__.get("_banddecode_launches", 0)
        if reset:
            self.__dict__["_banddecode_launches"] = 0
        return rc

    def pdnv_decode_attention_supported(self, H, Hkv, hd, NS, window, max_len):
        if min(H, Hkv, hd, max_len, window) <= 0 or H % Hkv or H // Hkv > 8 or hd % 4 or hd > 128 or not 1 <= NS <= 64:
            return 0
        G, chunk = H // Hkv, -(-(-(-min(window, max_len) // NS)) // 4) * 4
        return int(4 * (G * hd + 2 * hd + 64 + max(G * chunk, G * (256 // (hd // 4)) * hd)) <= 60 * 1024)

    def pdnv_decode_attention_f32(self, qkv, rs, cos, sin, kc, vc, parts, B, H, Hkv, hd, NS, cbs, pos, max_len, window,
                                  rows, stream):
        if B == 0 or H == 0:
            return 0
        if not (qkv and cos and sin and kc and vc and parts and pos and max_len > 0 and B > 0):
            return -1
        if not self.pdnv_decode_attention_supported(H, Hkv, hd, NS, window, max_len):
            return -2
        D, KVD, G, half = H * hd, Hkv * hd, H // Hkv, hd // 2
        if cbs % 4 or rs % 4 or ((qkv | kc | vc | parts) & 15) or rs < D + 2 * KVD or cbs < max_len * KVD:
            return -1
        x = view(qkv, (B, D + 2 * KVD), (rs, 1), np.float32)
        Kc, Vc = (view(p, (B, max_len, Hkv, hd), (cbs, KVD, hd, 1), np.float32) for p in (kc, vc))
        out = flat(parts, B * NS * H * (4 + hd)).reshape(B, NS, H, 4 + hd)
        P = flat(pos, B if rows else 1, np.int32)
        for b in range(B):
            pu = int(P[b if rows else 0])
            p = max(pu, 0)
            assert p < max_len
            lo = max(0, p - window + 1)               # (rows below lo are never touched: the window's keys alone)
            c, s = flat(cos + 4 * p * half, half), flat(sin + 4 * p * half, half)
            q = rotate(np.array(x[b, :D]).reshape(H, hd), c, s)
            K, V = np.array(Kc[b, lo:p + 1]), np.array(Vc[b, lo:p + 1])
            K[-1], V[-1] = rotate(np.array(x[b, D:D + KVD]).reshape(Hkv, hd), c, s), x[b, D + KVD:].reshape(Hkv, hd)
            if pu >= 0:                           # (a stopped row: position 0, its cache left alone)
                Kc[b, p], Vc[b, p] = K[-1], V[-1]
            sc = np.einsum("hd,thd->ht", q, np.repeat(K, G, axis=1)) / np.float32(math.sqrt(hd))
            Vr, n = np.repeat(V, G, axis=1), p - lo + 1
            chunk = -(-n // NS)                   # (the ranges cut the window: range sp = keys lo + [t0, t1))
            for sp in range(NS):
                t0, t1 = sp * chunk, min(n, (sp + 1) * chunk)
                out[b, sp, :, 4:] = 0.0
                out[b, sp, :, 0], out[b, sp, :, 1] = -np.inf, 0.0
                if t0 < t1:
                    m = sc[:, t0:t1].max(-1)
                    e = np.exp(sc[:, t0:t1] - m[:, None])
                    out[b, sp, :, 0], out[b, sp, :, 1] = m, e.sum(-1)
                    out[b, sp, :, 4:] = np.einsum("ht,thd->hd", e, Vr[t0:t1])
        self.__dict__["_banddecode_launches"] = self.__dict__.get("_banddecode_launches", 0) + 1
        return 0


def extend():
    """Make the installed emulator answer the pdnv_ entries as well; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, BandDecodeMixin):
        emu.__class__ = type("BandDecode" + type(emu).__name__, (BandDecodeMixin, type(emu)), {})
        emu.protos.update(_lib.parse_header(_lib.BANDDECODE_HEADER_PATHS[0]))
    return emu
