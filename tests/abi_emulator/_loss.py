"""Cross entropy with ignore_index (csrc/masked_loss.hip): the entries of include/pdn_loss.h (prefix pdnl_).  As for the
pdnx_ entries (_optim.py) the core header's registry is closed to them, so this part carries its own: `LossMixin`, its
`NOT_EMULATED` and `extend()`.  tests/test_loss_abi_cpu.py holds header, exports and this part equal.  Every entry states
the contract through the product's float64 module, pydynet_amd/core/fused/masked_loss.py, rounded to float32.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.fused import masked_loss as M
from . import EmulatedLib
from ._base import flat, view

NOT_EMULATED = ()


def _sanitise(targets, rows, ignore, V, err):
    """targets with V on ignored rows and 0 (flag raised) on rows that are neither ignored nor a class"""
    t = np.array(flat(targets, rows, np.int64))
    valid = M.valid_rows(t, ignore)
    bad = valid & ((t < 0) | (t >= V))
    if bad.any():
        ctypes.cast(err, ctypes.POINTER(ctypes.c_int))[0] = 1
        t[bad] = 0
    t[~valid] = V
    return t


def _stats(stats, t_safe, V, mean):
    count, factor = M.scale(t_safe, V, "mean" if mean else "sum")
    s = flat(stats, 4)
    s[0], s[1] = count, factor
    return factor


def _lse(a):
    m = a.max(-1, keepdims=True)
    return (np.log(np.exp(a - m).sum(-1, keepdims=True)) + m)[:, 0]


class LossMixin:
    def pdnl_cross_entropy_colsum_workspace_bytes(self, rows, V):
        return 256 * V * 4 if (V >= 4096 and V % 4 == 0 and V <= 32768 and rows > 0) else 0

    def pdnl_cross_entropy_fwd_f32(self, logits, targets, ignore, rows, V, mean, loss_row, lse_row, loss_out, stats, err, stream):
        if not (rows > 0 and V > 0 and logits and targets and loss_row and lse_row and loss_out and stats and err):
            return -1
        a = flat(logits, rows * V).reshape(rows, V)
        t = _sanitise(targets, rows, ignore, V, err)
        _stats(stats, t, V, mean)
        valid = t != V
        flat(lse_row, rows)[...] = np.where(valid, _lse(a.astype(np.float64)), 0.0)
        ts = np.where(valid, t, 0)
        flat(loss_row, rows)[...] = np.where(valid, flat(lse_row, rows) - a[np.arange(rows), ts], 0.0)
        flat(loss_out, 1)[0] = M.cross_entropy(a, t, V, "mean" if mean else "sum")[0]
        return 0

    def pdnl_cross_entropy_fwd_bwd_f32(self, logits, targets, ignore, rows, V, mean, loss_row, lse_row, loss_out, stats,
                                       dlogits, colsum, ws, wsb, err, stream):
        if not dlogits:
            return -1
        if colsum and not self.pdnl_cross_entropy_colsum_workspace_bytes(rows, V):
            return -2
        if colsum and (not ws or wsb < self.pdnl_cross_entropy_colsum_workspace_bytes(rows, V)):
            return -3
        rc = self.pdnl_cross_entropy_fwd_f32(logits, targets, ignore, rows, V, mean, loss_row, lse_row, loss_out, stats, err, stream)
        if rc:
            return rc
        a = flat(logits, rows * V).reshape(rows, V)
        d = M.cross_entropy(a, _sanitise(targets, rows, ignore, V, err), V, "mean" if mean else "sum")[1].astype(np.float32)
        flat(dlogits, rows * V).reshape(rows, V)[...] = d
        if colsum:
            flat(colsum, V)[...] = d.sum(0)
        return 0

    def pdnl_cross_entropy_bwd_f32(self, logits, targets, ignore, lse_row, upstream, stats, dlogits, rows, V, stream):
        if rows == 0:
            return 0
        a = flat(logits, rows * V).reshape(rows, V)
        t = np.array(flat(targets, rows, np.int64))
        t[~M.valid_rows(t, ignore)] = V
        g = float(flat(upstream, 1)[0]) if upstream else 1.0
        d = M.cross_entropy(a, np.where((t < 0) | (t > V), 0, t), V, "sum", g * float(flat(stats, 4)[1]))[1]
        flat(dlogits, rows * V).reshape(rows, V)[...] = d
        return 0

    def pdnl_linear_ce_finish_f32(self, logits, ldl, lse, targets, ignore, rows, V, mean, loss_row, loss_out, stats, safe, err,
                                  stream):
        if not (rows > 0 and V > 0 and ldl >= V and logits and lse and targets and loss_row and loss_out and stats and safe and err):
            return -1
        z = view(logits, (rows, V), (ldl, 1), np.float32)
        t = _sanitise(targets, rows, ignore, V, err)
        factor = _stats(stats, t, V, mean)
        valid = t != V
        ls = flat(lse, rows)
        lr = np.where(valid, ls - z[np.arange(rows), np.where(valid, t, 0)], np.float32(0))
        flat(loss_row, rows)[...] = lr
        flat(loss_out, 1)[0] = lr.sum(dtype=np.float32) * np.float32(factor)
        ls[~valid] = np.inf
        flat(safe, rows, np.int64)[...] = t
        return 0

    def pdnl_linear_ce_backward_f32(self, x, ldx, logits, lse, safe, stats, upstream, W, dx, dxd, dW, dw_beta, dbias, db_beta,
                                    rows, V, fin, ws, wsb, stream):
        if rows == 0 or V == 0:
            return 0
        if not (x and logits and lse and safe and stats and W) or (dx and dxd):
            return -1
        if (dx or dW or dbias) and not self.pdn_linear_ce_supported(rows, V, fin):
            return -2
        if dW or dbias:
            self._count(13)
        s = flat(stats, 4)
        s[2] = (flat(upstream, 1)[0] if upstream else np.float32(1)) * s[1]
        t = flat(safe, rows, np.int64)
        # the statement's dlogits from the saved logits ('sum' with the device scalar as upstream: the factor is inside it)
        d = M.cross_entropy(flat(logits, rows * V).reshape(rows, V), t, V, "sum", float(s[2]))[1].astype(np.float32)
        xv = view(x, (rows, fin), (ldx, 1), np.float32)
        w = flat(W, fin * V).reshape(fin, V)
        if dx:
            flat(dx, rows * fin).reshape(rows, fin)[...] = d @ w.T
        if dxd:
            r = flat(dxd, rows * fin).reshape(rows, fin)
            r *= s[2]
            r[t == V] = 0.0
        if dW:
            g = flat(dW, fin * V).reshape(fin, V)
            g[...] = np.float32(dw_beta) * g + xv.T @ d if dw_beta != 0.0 else xv.T @ d
        if dbias:
            bg = flat(dbias, V)
            bg[...] = np.float32(db_beta) * bg + d.sum(0) if db_beta != 0.0 else d.sum(0)
        return 0


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnl_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library.  (`_optim.extend()` replaces the
    class: call it first where both are needed.)"""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, LossMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("Loss" + base.__name__, (LossMixin, base), {"__doc__": "with the entries of include/pdn_loss.h"})
        emu.__class__ = _classes[base]
        for path in _lib.LOSS_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
