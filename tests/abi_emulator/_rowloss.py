"""Cross entropy with reduction='none' (csrc/row_loss.hip): the entries of include/pdn_rowloss.h (prefix pdnr_).  As for the
pdnx_, pdnl_ and pdns_ entries (_optim.py, _loss.py, _segattn.py) the core header's registry is closed to them, so this part
carries its own: `RowLossMixin`, its `NOT_EMULATED` and `extend()`.  tests/test_rowloss_abi_cpu.py holds header, exports and
this part equal.  Every entry states the contract through the product's float64 module,
pydynet_amd/core/fused/row_loss.py, rounded to float32.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.fused import row_loss as R
from . import EmulatedLib
from ._base import flat, view

NOT_EMULATED = ()
ROW_SLOT = 44                                    # PDN_CNT_ROW_LOSS of csrc/common.h


def _colsum_bytes(rows, V):
    return max(1, min(2048, (rows + 63) // 64)) * V * 4 if (rows > 0 and V > 0) else 0


class RowLossMixin:
    # launch counter slot 44 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == ROW_SLOT:
            self.__dict__["_row_launches"] = self.__dict__.get("_row_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > ROW_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[ROW_SLOT] = self.__dict__.get("_row_launches", 0)
        if reset:
            self.__dict__["_row_launches"] = 0
        return rc

    def pdnr_cross_entropy_bwd_rows_f32(self, logits, targets, masked, ignore, lse_row, u, dlogits, rows, V, stream):
        if rows == 0:
            return 0
        if not (logits and targets and lse_row and u and dlogits and V > 0 and rows > 0):
            return -1
        self._count(ROW_SLOT)
        a = flat(logits, rows * V).reshape(rows, V)
        t = np.array(flat(targets, rows, np.int64))
        valid = R.valid_rows(t, ignore if masked else None)
        if not masked:
            t[t < 0] += V                                 # (the unmasked forward wraps a negative target)
        t = np.where(valid & (t >= 0) & (t < V), t, 0)    # (a bad target was flagged by the forward pass)
        d = R.dlogits(a, np.where(valid, t, -1), np.array(flat(u, rows)), -1)
        flat(dlogits, rows * V).reshape(rows, V)[...] = d
        return 0

    def pdnr_linear_ce_finish_rows_f32(self, logits, ldl, lse, targets, masked, ignore, rows, V, loss_row, safe, err, stream):
        if not (rows > 0 and V > 0 and ldl >= V and logits and lse and targets and loss_row and safe and err):
            return -1
        self._count(ROW_SLOT)
        z = view(logits, (rows, V), (ldl, 1), np.float32)
        t = np.array(flat(targets, rows, np.int64))
        valid = R.valid_rows(t, ignore if masked else None)
        bad = valid & ((t < 0) | (t >= V))
        if bad.any():
            ctypes.cast(err, ctypes.POINTER(ctypes.c_int))[0] = 1
            t[bad] = 0
        t[~valid] = V
        ls = flat(lse, rows)
        flat(loss_row, rows)[...] = np.where(valid, ls - z[np.arange(rows), np.where(valid, t, 0)], np.float32(0))
        ls[~valid] = np.inf
        flat(safe, rows, np.int64)[...] = t
        return 0

    def pdnr_scale_rows_f32(self, src, ld_in, out, ld_out, rows, cols, u, inv_s, safe, V, stream):
        if rows == 0 or cols == 0:
            return 0
        if not (src and out and u and safe and ld_in >= cols and ld_out >= cols):
            return -1
        self._count(ROW_SLOT)
        self._scale_rows(src, ld_in, out, ld_out, rows, cols, u, inv_s, safe, V)
        return 0

    @staticmethod
    def _scale_rows(src, ld_in, out, ld_out, rows, cols, u, inv_s, safe, V):
        keep = flat(safe, rows, np.int64) != V
        a = np.array(view(src, (rows, cols), (ld_in, 1), np.float32))
        r = R.scale_rows(a, np.array(flat(u, rows)), keep, float(flat(inv_s, 1)[0]) if inv_s else 1.0)
        view(out, (rows, cols), (ld_out, 1), np.float32)[...] = r

    @staticmethod
    def _abs_max(u, safe, V, rows, s_out):
        s, inv = R.abs_max(np.array(flat(u, rows)), flat(safe, rows, np.int64) != V)
        o = flat(s_out, 2)
        o[0], o[1] = s, np.float32(1) / np.float32(s) if s > 0 else 0.0

    def pdnr_abs_max_rows_f32(self, u, safe, V, rows, s_out, stream):
        if not (u and safe and s_out and rows >= 0):
            return -1
        self._count(ROW_SLOT)
        self._abs_max(u, safe, V, rows, s_out)
        return 0

    def pdnr_weighted_colsum_workspace_bytes(self, rows, V):
        return _colsum_bytes(rows, V)

    @staticmethod
    def _dz(logits, ldl, lse, safe, u, rows, V):
        """the statement's dlogits from the saved logits and the masked lse (+inf on ignored rows)"""
        z = np.array(view(logits, (rows, V), (ldl, 1), np.float32), np.float64)
        t = flat(safe, rows, np.int64)
        keep = t != V
        d = np.exp(z - np.where(keep, np.array(flat(lse, rows), np.float64), 0.0)[:, None])
        d[np.arange(rows), np.where(keep, t, 0)] -= 1.0
        d *= np.where(keep, np.array(flat(u, rows), np.float64), 0.0)[:, None]
        d[~keep] = 0.0
        return d

    def _colsum(self, logits, ldl, lse, safe, u, rows, V, dbias, db_beta, ws, wsb):
        if not ws or wsb < _colsum_bytes(rows, V):
            return -3
        bg = flat(dbias, V)
        s = self._dz(logits, ldl, lse, safe, u, rows, V).sum(0)
        bg[...] = np.float32(db_beta) * bg + s if db_beta != 0.0 else s
        return 0

    def pdnr_weighted_colsum_f32(self, logits, ldl, lse, safe, u, rows, V, dbias, db_beta, ws, wsb, stream):
        if not (logits and lse and safe and u and dbias and rows > 0 and V > 0 and ldl >= V):
            return -1
        self._count(ROW_SLOT)
        return self._colsum(logits, ldl, lse, safe, u, rows, V, dbias, db_beta, ws, wsb)

    def pdnr_linear_ce_backward_rows_f32(self, x, ldx, logits, lse, safe, u, W, dx, dxd, dW, dw_beta, dbias, db_beta, xs, s_out,
                                         rows, V, fin, ws, wsb, cws, cwsb, stream):
        if rows == 0 or V == 0:
            return 0
        if not (x and logits and lse and safe and u and W) or (dx and dxd) or (dW and not (xs and s_out)):
            return -1
        if (dx or dW) and not self.pdn_linear_ce_supported(rows, V, fin):
            return -2
        self._count(ROW_SLOT)
        if dbias:
            rc = self._colsum(logits, V, lse, safe, u, rows, V, dbias, db_beta, cws, cwsb)
            if rc:
                return rc
        w = np.array(flat(W, fin * V).reshape(fin, V), np.float64)
        if dx:
            flat(dx, rows * fin).reshape(rows, fin)[...] = self._dz(logits, V, lse, safe, u, rows, V) @ w.T
        if dxd:
            self._scale_rows(dxd, fin, dxd, fin, rows, fin, u, None, safe, V)
        if dW:
            if not ws or wsb <= 0:
                return -3
            self._count(13)
            # as the library: the scaled copy of x against s * (softmax - onehot)
            self._abs_max(u, safe, V, rows, s_out)
            self._scale_rows(x, ldx, xs, fin, rows, fin, u, int(s_out) + 4, safe, V)
            s = float(flat(s_out, 2)[0])
            ones = np.ones(rows, np.float32)
            dz = self._dz(logits, V, lse, safe, ones.ctypes.data, rows, V) * s
            g = flat(dW, fin * V).reshape(fin, V)
            prod = np.array(flat(xs, rows * fin).reshape(rows, fin), np.float64).T @ dz
            g[...] = np.float32(dw_beta) * g + prod if dw_beta != 0.0 else prod
        return 0


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnr_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, RowLossMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("Row" + base.__name__, (RowLossMixin, base), {"__doc__": "with the entries of include/pdn_rowloss.h"})
        emu.__class__ = _classes[base]
        for path in _lib.ROWLOSS_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
