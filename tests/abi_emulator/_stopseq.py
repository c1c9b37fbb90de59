"""Multi-token stop sequences of a decode step (csrc/stop_seq.hip): the entries of include/pdn_stopseq.h (prefix pdnh_).
As for the pdnf_ entries and the parts before them the core header's registry is closed to them, so this part carries its
own: `StopSeqMixin`, its `NOT_EMULATED` and `extend()`.  tests/test_stopseq_abi_cpu.py holds header, exports and this part
equal.  Every entry states the contract through the product's module, pydynet_amd/llm/stop_sequences.py; `stop_step_np` /
`stop_reset_np` are also the references of the GPU tests.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.llm import stop_sequences as SS
from . import EmulatedLib
from ._base import flat

NOT_EMULATED = ()
STOPSEQ_SLOT = 53                                # PDN_CNT_STOP_SEQ of csrc/common.h
ROWS_PER_GROUP = 4                               # rows per workgroup of csrc/stop_seq.hip, one wave each


def stop_step_np(ids, pos, tables, sets, start, tail, min_new):
    """pdnh_stop_step on arrays: ids (B,) the tokens the tick stored, pos (B,) the positions it left (in place: -1 for the
    rows that stop), tables = (set_off, seq_off, toks), sets / start (B,), tail (B, 16) (in place), min_new an int."""
    n_sets = tables[0].size - 1
    for b in range(pos.size):
        p, s = int(pos[b]), int(sets[b])
        g = p - int(start[b])
        if p < 0 or s < 0 or s >= n_sets or g < 1:
            continue
        t = int(ids[b])
        tok = t if 0 <= t <= 0x7fffffff else -1
        hit = SS.match(_first16(tables, s), 0, tail[b], g, tok)
        tail[b, g % SS.MAX_LEN] = tok
        if hit and g > min_new:
            pos[b] = -1


def _first16(tables, s):
    """Set s of the tables alone, cut to the 16 sequences the kernel looks at, offsets clamped as the kernel clamps them."""
    set_off, seq_off, toks = tables
    n_seqs, n_toks = seq_off.size - 1, toks.size
    q0 = min(max(int(set_off[s]), 0), n_seqs)
    q1 = min(max(int(set_off[s + 1]), q0), n_seqs)
    seqs = []
    for q in range(q0, min(q1, q0 + SS.MAX_SEQS)):
        lo = min(max(int(seq_off[q]), 0), n_toks)
        seqs.append(toks[lo:min(max(int(seq_off[q + 1]), lo), n_toks)])
    return SS.packed([seqs])


def stop_reset_np(state, rows, src):
    """pdnh_stop_reset on arrays (in place): state = (set (B,), start (B,), tail (B, 16)), src = (sets (R,), prompt lengths
    (R,), first tokens (R,), -1: none)."""
    sets, start, tail = state
    for i, b in enumerate(np.asarray(rows).tolist()):
        if 0 <= b < sets.shape[0]:
            sets[b], start[b] = src[0][i], src[1][i]
            tail[b] = -1
            if src[2][i] >= 0:
                tail[b, 1] = src[2][i]


class StopSeqMixin:
    # launch counter slot 53 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == STOPSEQ_SLOT:
            self.__dict__["_stopseq_launches"] = self.__dict__.get("_stopseq_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > STOPSEQ_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[STOPSEQ_SLOT] = self.__dict__.get("_stopseq_launches", 0)
        if reset:
            self.__dict__["_stopseq_launches"] = 0
        return rc

    def pdnh_stop_reset(self, sets, start, tail, B, rows, n_rows, s_set, s_start, s_first, stream):
        if n_rows == 0:
            return 0
        if not (sets and start and tail and rows and s_set and s_start and s_first and B > 0 and n_rows > 0):
            return -1
        R = n_rows
        stop_reset_np((flat(sets, B, np.int32), flat(start, B, np.int32),
                       flat(tail, B * SS.MAX_LEN, np.int32).reshape(B, SS.MAX_LEN)), np.array(flat(rows, R, np.int32)),
                      tuple(np.array(flat(a, R, np.int32)) for a in (s_set, s_start, s_first)))
        self._count(STOPSEQ_SLOT)
        return 0

    def pdnh_stop_step(self, ids, pos, B, set_off, seq_off, toks, n_sets, n_seqs, n_toks, sets, start, tail, min_new,
                       stream):
        if B == 0:
            return 0
        if not (ids and pos and set_off and seq_off and toks and sets and start and tail and min_new and B > 0
                and n_sets > 0 and n_seqs > 0 and n_toks > 0):
            return -1
        tables = (np.array(flat(set_off, n_sets + 1, np.int32)), np.array(flat(seq_off, n_seqs + 1, np.int32)),
                  np.array(flat(toks, n_toks, np.int32)))
        stop_step_np(np.array(flat(ids, B, np.int64)), flat(pos, B, np.int32), tables, np.array(flat(sets, B, np.int32)),
                     np.array(flat(start, B, np.int32)), flat(tail, B * SS.MAX_LEN, np.int32).reshape(B, SS.MAX_LEN),
                     int(flat(min_new, 1, np.int32)[0]))
        self._count(STOPSEQ_SLOT)
        return 0


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnh_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, StopSeqMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("StopSeq" + base.__name__, (StopSeqMixin, base),
                                  {"__doc__": "with the entries of include/pdn_stopseq.h"})
        emu.__class__ = _classes[base]
        for path in _lib.STOPSEQ_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
