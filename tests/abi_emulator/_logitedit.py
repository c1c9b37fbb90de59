"""Per-request logit edits of a decode step (csrc/logit_edit.hip): the entries of include/pdn_logitedit.h (prefix pdne_).
As for the pdnx_, pdnl_, pdns_, pdnr_ and pdnz_ entries (_optim.py, _loss.py, _segattn.py, _rowloss.py, _smoothloss.py) the
core header's registry is closed to them, so this part carries its own: `LogitEditMixin`, its `NOT_EMULATED` and `extend()`.
tests/test_logitedit_abi_cpu.py holds header, exports and this part equal.  Every entry states the contract through the
product's module, pydynet_amd/llm/logit_edits.py; `edit_np` / `edit_reset_np` are also the references of the GPU tests.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.llm import logit_edits as E
from . import EmulatedLib
from ._base import flat, view

NOT_EMULATED = ()
EDIT_SLOT = 48                                   # PDN_CNT_LOGIT_EDIT of csrc/common.h
EDIT_CHUNK = 1024                                # vocabulary tokens per workgroup of csrc/logit_edit.hip


def edit_chunks(V):
    return -(-V // EDIT_CHUNK) if V > 0 else 0


def candidates_np(z):
    """Each 1024-token chunk's first maximum and its index, (B, n) each: a NaN never wins against a number, a chunk of
    nothing but NaN yields (NaN, its first index)."""
    B, V = z.shape
    n = edit_chunks(V)
    cv, ci = np.zeros((B, n), np.float32), np.zeros((B, n), np.int32)
    for b in range(B):
        for j in range(n):
            seg = z[b, j * EDIT_CHUNK:(j + 1) * EDIT_CHUNK]
            if np.isnan(seg).all():
                cv[b, j], ci[b, j] = np.nan, j * EDIT_CHUNK
                continue
            k = int(np.argmax(np.where(np.isnan(seg), -np.inf, seg)))
            cv[b, j], ci[b, j] = seg[k], j * EDIT_CHUNK + k
    return cv, ci


def edit_np(z, m=0, allow=None, allow_on=None, ids=None, vals=None, cnt=None, generated=None, pos=None, stop=None):
    """Either edit entry on arrays: z (B, V) float32 edited in place (rows with pos < 0 untouched) from the packed state
    -- allow (B, W) int32 with allow_on (B,), the bias tables ids / vals (B, MAX_BIAS) with cnt (B,), generated (B,),
    stop (W,) int32; each may be None.  Returns (live rows (B,) bool, candidate values (B, n), candidate indices (B, n))."""
    B, V = z.shape
    live = np.ones(B, bool) if pos is None else np.asarray(pos).reshape(-1) >= 0
    rows = np.flatnonzero(live)
    if rows.size:
        a = [None] * rows.size if allow is None else E.bits_allow(np.asarray(allow)[rows], np.asarray(allow_on)[rows], V)
        t = None if cnt is None else E.tables_bias(np.asarray(ids)[rows], np.asarray(vals)[rows], np.asarray(cnt)[rows])
        g = None if generated is None else np.asarray(generated)[rows]
        stops = () if stop is None else E.bits_allow(np.asarray(stop).reshape(1, -1), [1], V)[0]
        z[rows] = E.apply(z[rows], a, t, g, int(m), stops)
    cv, ci = candidates_np(z)
    return live, cv, ci


def edit_reset_np(state, rows, src):
    """pdne_logit_edit_reset on arrays (in place): state = (allow (B, W), allow_on, ids (B, MAX_BIAS), vals, cnt, start),
    src = (allow (R, W) or None, on or None, ids or None, vals or None, cnt or None, start (R,))."""
    allow, on, ids, vals, cnt, start = state
    s_allow, s_on, s_ids, s_vals, s_cnt, s_start = src
    B = on.shape[0]
    for i, b in enumerate(np.asarray(rows).tolist()):
        if not 0 <= b < B:
            continue
        o = int(s_on[i] != 0) if s_allow is not None else 0
        if o:
            allow[b] = s_allow[i]
        n = min(max(int(s_cnt[i]), 0), E.MAX_BIAS) if s_cnt is not None else 0
        if n:
            ids[b, :n], vals[b, :n] = s_ids[i, :n], s_vals[i, :n]
        on[b], cnt[b], start[b] = o, n, s_start[i]


class LogitEditMixin:
    # launch counter slot 48 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == EDIT_SLOT:
            self.__dict__["_edit_launches"] = self.__dict__.get("_edit_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > EDIT_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[EDIT_SLOT] = self.__dict__.get("_edit_launches", 0)
        if reset:
            self.__dict__["_edit_launches"] = 0
        return rc

    def pdne_logit_edit_chunks(self, V):
        return edit_chunks(V)

    def pdne_logit_edit_reset(self, allow, allow_on, bias_ids, bias_val, bias_n, start, B, V, rows, n_rows, s_allow, s_on,
                              s_ids, s_val, s_n, s_start, stream):
        if n_rows == 0:
            return 0
        if not (allow and allow_on and bias_ids and bias_val and bias_n and start and rows and s_start and B > 0 and V > 0
                and n_rows > 0 and bool(s_allow) == bool(s_on) and bool(s_ids) == bool(s_n) and bool(s_val) == bool(s_n)):
            return -1
        W, M, R = -(-V // 32), E.MAX_BIAS, n_rows
        state = (flat(allow, B * W, np.int32).reshape(B, W), flat(allow_on, B, np.int32),
                 flat(bias_ids, B * M, np.int32).reshape(B, M), flat(bias_val, B * M).reshape(B, M),
                 flat(bias_n, B, np.int32), flat(start, B, np.int32))
        src = (np.array(flat(s_allow, R * W, np.int32)).reshape(R, W) if s_allow else None,
               np.array(flat(s_on, R, np.int32)) if s_on else None,
               np.array(flat(s_ids, R * M, np.int32)).reshape(R, M) if s_ids else None,
               np.array(flat(s_val, R * M)).reshape(R, M) if s_val else None,
               np.array(flat(s_n, R, np.int32)) if s_n else None, np.array(flat(s_start, R, np.int32)))
        edit_reset_np(state, np.array(flat(rows, R, np.int32)), src)
        self._count(EDIT_SLOT)
        return 0

    def _edit(self, logits, rs, B, V, params, allow, allow_on, bias_ids, bias_val, bias_n, generated, pos, stop, cand_v,
              cand_i):
        W, M = -(-V // 32), E.MAX_BIAS
        Z = view(logits, (B, V), (rs, 1), np.float32)
        z = np.array(Z)
        live, cv, ci = edit_np(
            z, int(flat(params, 4, np.int32)[0]),
            np.array(flat(allow, B * W, np.int32)).reshape(B, W) if allow else None,
            np.array(flat(allow_on, B, np.int32)) if allow_on else None,
            np.array(flat(bias_ids, B * M, np.int32)).reshape(B, M) if bias_ids else None,
            np.array(flat(bias_val, B * M)).reshape(B, M) if bias_val else None,
            np.array(flat(bias_n, B, np.int32)) if bias_n else None, generated, pos,
            np.array(flat(stop, W, np.int32)) if stop else None)
        Z[...] = z
        if cand_v:
            n = edit_chunks(V)
            V_, I_ = flat(cand_v, B * n, np.float32).reshape(B, n), flat(cand_i, B * n, np.int32).reshape(B, n)
            V_[live], I_[live] = cv[live], ci[live]
        self._count(EDIT_SLOT)
        return 0

    def pdne_logit_edit_step_f32(self, logits, rs, B, V, params, allow, allow_on, bias_ids, bias_val, bias_n, start, pos,
                                 pos_per_row, stop, cand_v, cand_i, stream):
        if B == 0:
            return 0
        if not (logits and params and allow and allow_on and bias_ids and bias_val and bias_n and start and pos and B > 0
                and V > 0 and rs >= V and bool(cand_v) == bool(cand_i)):
            return -1
        P = np.array(flat(pos, B if pos_per_row else 1, np.int32))
        P = P if pos_per_row else np.full(B, P[0])
        return self._edit(logits, rs, B, V, params, allow, allow_on, bias_ids, bias_val, bias_n,
                          P - np.array(flat(start, B, np.int32)), P, stop, cand_v, cand_i)

    def pdne_logit_edit_rows_f32(self, logits, rs, B, V, params, allow, allow_on, bias_ids, bias_val, bias_n, generated, pos,
                                 stop, cand_v, cand_i, stream):
        if B == 0:
            return 0
        if not (logits and params and B > 0 and V > 0 and rs >= V and bool(cand_v) == bool(cand_i)
                and bool(allow) == bool(allow_on) and bool(bias_ids) == bool(bias_n) and bool(bias_val) == bool(bias_n)):
            return -1
        return self._edit(logits, rs, B, V, params, allow, allow_on, bias_ids, bias_val, bias_n,
                          np.array(flat(generated, B, np.int32)) if generated else None,
                          np.array(flat(pos, B, np.int32)) if pos else None, stop, cand_v, cand_i)


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdne_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, LogitEditMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("Edit" + base.__name__, (LogitEditMixin, base),
                                  {"__doc__": "with the entries of include/pdn_logitedit.h"})
        emu.__class__ = _classes[base]
        for path in _lib.EDIT_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
