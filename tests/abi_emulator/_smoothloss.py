"""Cross entropy with label_smoothing and z_loss (csrc/smooth_loss.hip): the entries of include/pdn_smoothloss.h (prefix
pdnz_).  As for the pdnx_, pdnl_, pdns_ and pdnr_ entries (_optim.py, _loss.py, _segattn.py, _rowloss.py) the core header's
registry is closed to them, so this part carries its own: `SmoothLossMixin`, its `NOT_EMULATED` and `extend()`.
tests/test_smoothloss_abi_cpu.py holds header, exports and this part equal.  Every entry states the contract through the
product's float64 module, pydynet_amd/core/fused/smooth_loss.py, rounded to float32.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.fused import smooth_loss as S
from . import EmulatedLib
from ._base import flat, view

NOT_EMULATED = ()
SMOOTH_SLOT = 45                                 # PDN_CNT_SMOOTH_LOSS of csrc/common.h
REDUCTIONS = {1: "sum", 2: "mean"}


def _sanitise(targets, rows, masked, ignore, V, err):
    """targets with V on ignored rows and 0 (flag raised) on valid rows that are not a class"""
    t = np.array(flat(targets, rows, np.int64))
    valid = np.ones(rows, bool) if not masked else t != ignore
    bad = valid & ((t < 0) | (t >= V))
    if bad.any():
        if err:
            ctypes.cast(err, ctypes.POINTER(ctypes.c_int))[0] = 1
        t[bad] = 0
    t[~valid] = V
    return t


def _reduce(loss_row, t_safe, V, reduction, loss_out, stats):
    count = int((t_safe != V).sum())
    factor = 1.0 if reduction == 1 else (1.0 / count if count else 0.0)
    s = flat(stats, 4)
    s[0], s[1] = count, factor
    flat(loss_out, 1)[0] = np.float32(loss_row.sum() * factor)


def _upstream(u, upstream, stats, rows):
    if u:
        return np.array(flat(u, rows), np.float64)
    g = float(flat(upstream, 1)[0]) if upstream else 1.0
    return np.full(rows, g * (float(flat(stats, 4)[1]) if stats else 1.0))


def _esum_bytes(rows, fin):
    if rows <= 0 or fin <= 0:
        return 0
    want = max(1, min(1024, (rows + 63) // 64))
    rps = (rows + want - 1) // want
    return ((rows + rps - 1) // rps + 1) * (fin + 1) * 4


class SmoothLossMixin:
    # launch counter slot 45 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == SMOOTH_SLOT:
            self.__dict__["_smooth_launches"] = self.__dict__.get("_smooth_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > SMOOTH_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[SMOOTH_SLOT] = self.__dict__.get("_smooth_launches", 0)
        if reset:
            self.__dict__["_smooth_launches"] = 0
        return rc

    def pdnz_cross_entropy_fwd_f32(self, logits, targets, masked, ignore, rows, V, reduction, eps, lam, loss_row, lse_row,
                                   loss_out, stats, err, stream):
        if not (rows > 0 and V > 0 and 0 <= reduction <= 2 and logits and targets and loss_row and lse_row and err
                and (reduction == 0 or (loss_out and stats))):
            return -1
        self._count(SMOOTH_SLOT)
        a = np.array(flat(logits, rows * V).reshape(rows, V), np.float64)
        t = _sanitise(targets, rows, masked, ignore, V, err)
        valid = t != V
        flat(lse_row, rows)[...] = np.where(valid, S._lse(a), 0.0)
        r = S.rows(a, t, eps, lam, V)
        flat(loss_row, rows)[...] = r
        if reduction:
            _reduce(r, t, V, reduction, loss_out, stats)
        return 0

    def pdnz_cross_entropy_bwd_f32(self, logits, targets, masked, ignore, lse_row, u, upstream, stats, eps, lam, dlogits, rows,
                                   V, stream):
        if rows == 0:
            return 0
        if not (logits and targets and lse_row and dlogits and V > 0 and rows > 0):
            return -1
        self._count(SMOOTH_SLOT)
        a = np.array(flat(logits, rows * V).reshape(rows, V), np.float64)
        t = _sanitise(targets, rows, masked, ignore, V, None)       # (a bad target was flagged by the forward pass)
        flat(dlogits, rows * V).reshape(rows, V)[...] = S.dlogits(a, t, _upstream(u, upstream, stats, rows), eps, lam, V)
        return 0

    def pdnz_weight_sums_f32(self, W, bias, fin, V, wsum, stream):
        if not (W and wsum and fin > 0 and V > 0):
            return -1
        self._count(SMOOTH_SLOT)
        ws, bs = S.weight_sums(flat(W, fin * V).reshape(fin, V), flat(bias, V) if bias else None)
        o = flat(wsum, fin + 1)
        o[:fin], o[fin] = ws, bs
        return 0

    def pdnz_linear_ce_finish_f32(self, logits, ldl, lse, targets, masked, ignore, x, ldx, wsum, rows, V, fin, reduction, eps,
                                  lam, loss_row, loss_out, stats, safe, err, stream):
        if not (rows > 0 and V > 0 and ldl >= V and 0 <= reduction <= 2 and logits and lse and targets and loss_row and safe
                and err and (reduction == 0 or (loss_out and stats))):
            return -1
        if eps != 0.0 and not (x and wsum and fin > 0 and ldx >= fin):
            return -1
        self._count(SMOOTH_SLOT)
        z = view(logits, (rows, V), (ldl, 1), np.float32)
        t = _sanitise(targets, rows, masked, ignore, V, err)
        valid = t != V
        ls = flat(lse, rows)
        l = np.where(valid, np.array(ls, np.float64), 0.0)
        zmean = 0.0
        if eps != 0.0:
            w = np.array(flat(wsum, fin + 1), np.float64)
            zmean = (np.array(view(x, (rows, fin), (ldx, 1), np.float32), np.float64) @ w[:fin] + w[fin]) / V
        r = np.where(valid, l - (1.0 - eps) * z[np.arange(rows), np.where(valid, t, 0)] - eps * zmean + lam * l * l, 0.0)
        flat(loss_row, rows)[...] = r
        if reduction:
            _reduce(r, t, V, reduction, loss_out, stats)
        ls[~valid] = np.inf
        flat(safe, rows, np.int64)[...] = t
        return 0

    def pdnz_row_coefficients_f32(self, lse, safe, u, upstream, stats, eps, lam, rows, V, u_out, c_out, e_out, stream):
        if rows == 0:
            return 0
        if not (lse and safe and u_out and c_out and e_out and rows > 0 and V > 0):
            return -1
        self._count(SMOOTH_SLOT)
        keep = flat(safe, rows, np.int64) != V
        up, c, e = S.coefficients(flat(lse, rows), keep, _upstream(u, upstream, stats, rows), eps, lam, V)
        flat(u_out, rows)[...], flat(c_out, rows)[...], flat(e_out, rows)[...] = up, c, e
        return 0

    def pdnz_linear_ce_corrections_workspace_bytes(self, rows, V, fin):
        return _esum_bytes(rows, fin) if V > 0 else 0

    def pdnz_linear_ce_corrections_f32(self, x, ldx, W, wsum, safe, c, e, dx, dW, dbias, rows, V, fin, ws, wsb, stream):
        if rows == 0 or V == 0:
            return 0
        if not (x and W and safe and c and rows > 0 and V > 0 and fin > 0 and ldx >= fin) or (e and not wsum):
            return -1
        if fin + 2 > 14336:
            return -2
        self._count(SMOOTH_SLOT)
        t = flat(safe, rows, np.int64)
        keep = t != V
        ts = np.where(keep, t, 0)
        cv = np.where(keep, np.array(flat(c, rows), np.float64), 0.0)
        ev = np.where(keep, np.array(flat(e, rows), np.float64), 0.0) if e else None
        xv = np.array(view(x, (rows, fin), (ldx, 1), np.float32), np.float64)
        w = flat(W, fin * V).reshape(fin, V)
        if dx:
            d = flat(dx, rows * fin).reshape(rows, fin)
            add = cv[:, None] * w[:, ts].T.astype(np.float64)
            if ev is not None:
                add -= ev[:, None] * np.array(flat(wsum, fin), np.float64)[None, :]
            d[keep] = (d + add)[keep]
        if not (dW or dbias):
            return 0
        if ev is not None and (not ws or wsb < _esum_bytes(rows, fin)):
            return -3
        if dW:
            col = np.zeros((V, fin))
            np.add.at(col, ts, cv[:, None] * xv)
            if ev is not None:
                col -= (ev[:, None] * xv).sum(0)[None, :]
            g = flat(dW, fin * V).reshape(fin, V)
            g[...] = g + col.T
        if dbias:
            col = np.zeros(V)
            np.add.at(col, ts, cv)
            if ev is not None:
                col -= ev.sum()
            bg = flat(dbias, V)
            bg[...] = bg + col
        return 0


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnz_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, SmoothLossMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("Smooth" + base.__name__, (SmoothLossMixin, base),
                                  {"__doc__": "with the entries of include/pdn_smoothloss.h"})
        emu.__class__ = _classes[base]
        for path in _lib.SMOOTH_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
