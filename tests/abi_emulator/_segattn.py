"""Document-masked attention (the SEG kernels of csrc/attention.hip, csrc/segments.hip): the entries of
include/pdn_segattn.h (prefix pdns_).  As for the pdnx_ and pdnl_ entries (_optim.py, _loss.py) the core header's registry is
closed to them, so this part carries its own: `SegAttnMixin`, its `NOT_EMULATED` and `extend()`.
tests/test_segattn_abi_cpu.py holds header, exports and this part equal.  Every entry states the contract through the
product's float64 module, pydynet_amd/core/fused/segments.py, rounded to float32.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.fused import segments as S
from . import EmulatedLib
from ._base import flat, view

NOT_EMULATED = ()
SEG_SLOT = 43                                    # PDN_CNT_ATT_SEG of csrc/common.h


def _blhd(ptr, B, H, L, hd, rs, bs):
    return view(ptr, (B, L, H, hd), (bs, rs, hd, 1), np.float32)


def _tables(rc, rsn, L, hd):
    return flat(rc, L * hd // 2).reshape(L, hd // 2), flat(rsn, L * hd // 2).reshape(L, hd // 2)


class SegAttnMixin:
    # launch counter slot 43 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == SEG_SLOT:
            self.__dict__["_seg_launches"] = self.__dict__.get("_seg_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > SEG_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[SEG_SLOT] = self.__dict__.get("_seg_launches", 0)
        if reset:
            self.__dict__["_seg_launches"] = 0
        return rc

    def pdns_attention_supported(self, L, hd):
        return 1 if (hd in (48, 64) and L % 32 == 0 and 32 <= L <= 1024) else 0

    def pdns_segment_bounds_i32(self, seg, B, L, start, end, err, stream):
        if B == 0 or L == 0:
            return 0
        if not (seg and start and end and err):
            return -1
        if L > 4096:
            return -2
        ids = flat(seg, B * L, np.int32).reshape(B, L)
        if S.decreasing_rows(ids).any():
            ctypes.cast(err, ctypes.POINTER(ctypes.c_int))[0] = 1
        s, e = S.bounds(ids)
        flat(start, B * L, np.int32).reshape(B, L)[...] = s
        flat(end, B * L, np.int32).reshape(B, L)[...] = e
        return 0

    def pdns_attention_fwd_f32(self, q, k, v, o, lse, B, H, L, hd, rs, bs, ors, obs, rc, rsn, start, stream):
        if B == 0 or H == 0 or L == 0:
            return 0
        if not (q and k and v and o and lse and start) or bool(rc) != bool(rsn):
            return -1
        if not self.pdns_attention_supported(L, hd):
            return -2
        self._count(9)
        self._count(SEG_SLOT)
        Q, K, V = (np.array(_blhd(p, B, H, L, hd, rs, bs)) for p in (q, k, v))
        if rc:
            c, s = _tables(rc, rsn, L, hd)
            Q, K = S.rotate(Q, c, s), S.rotate(K, c, s)
        st = flat(start, B * L, np.int32).reshape(B, L)
        out, ls, _ = S.attention_forward(Q, K, V, st)
        _blhd(o, B, H, L, hd, ors, obs)[...] = out
        flat(lse, B * H * L).reshape(B, H, L)[...] = ls
        return 0

    def pdns_attention_bwd_f32(self, q, k, v, o, do, lse, dq, dk, dv, B, H, L, hd, rs, bs, ors, obs, rc, rsn, prerotated,
                               start, end, ws, wsb, stream):
        if B == 0 or H == 0 or L == 0:
            return 0
        if not (q and k and v and o and do and lse and dq and dk and dv and start and end) or bool(rc) != bool(rsn):
            return -1
        if prerotated and not rc:
            return -1
        if not self.pdns_attention_supported(L, hd):
            return -2
        if not ws or wsb < B * H * L * 4:
            return -3
        self._count(10)
        self._count(SEG_SLOT)
        Q, K, V = (np.array(_blhd(p, B, H, L, hd, rs, bs)) for p in (q, k, v))
        DO = np.array(_blhd(do, B, H, L, hd, ors, obs))
        if rc:
            c, s = _tables(rc, rsn, L, hd)
            if not prerotated:
                Q, K = S.rotate(Q, c, s), S.rotate(K, c, s)
        st = flat(start, B * L, np.int32).reshape(B, L)
        # (the visible range of a key follows from the queries' starts: seg_end is the same statement seen from the key)
        gq, gk, gv = S.attention_backward(Q, K, V, DO, st)
        if rc:
            gq, gk = S.rotate(gq, c, s, -1.0), S.rotate(gk, c, s, -1.0)
        _blhd(dq, B, H, L, hd, rs, bs)[...] = gq
        _blhd(dk, B, H, L, hd, rs, bs)[...] = gk
        _blhd(dv, B, H, L, hd, rs, bs)[...] = gv
        return 0


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdns_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, SegAttnMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("Seg" + base.__name__, (SegAttnMixin, base), {"__doc__": "with the entries of include/pdn_segattn.h"})
        emu.__class__ = _classes[base]
        for path in _lib.SEG_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
