"""Token-FSM constrained decoding of a decode step (csrc/token_fsm.hip): the entries of include/pdn_fsm.h (prefix pdnf_).
As for the pdnx_, pdnl_, pdns_, pdnr_, pdnz_, pdne_ and pdnq_ entries the core header's registry is closed to them, so this
part carries its own: `FsmMixin`, its `NOT_EMULATED` and `extend()`.  tests/test_fsm_abi_cpu.py holds header, exports and
this part equal.  Every entry states the contract through the product's module, pydynet_amd/llm/token_fsm.py; `fsm_np` /
`fsm_reset_np` are also the references of the GPU tests.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.llm import token_fsm as F
from . import EmulatedLib
from ._base import flat, view
from ._logitedit import candidates_np

NOT_EMULATED = ()
FSM_SLOT = 52                                    # PDN_CNT_TOKEN_FSM of csrc/common.h
FSM_CHUNK = 1024                                 # vocabulary tokens per workgroup of csrc/token_fsm.hip


def fsm_chunks(V):
    return -(-V // FSM_CHUNK) if V > 0 else 0


def fsm_np(z, tables, states=None, word=None, start_state=None, start=None, ids=None, pos=None):
    """Either masking entry on arrays: z (B, V) float32 masked in place (rows with pos < 0 untouched).  The rows form:
    `states` (B,) is given.  The step's form: the state words `word` (B,) int64, updated in place, with start_state, start,
    the fed ids and pos.  Returns (live rows (B,) bool, candidate values (B, n), candidate indices (B, n))."""
    B, V = z.shape
    pos = np.zeros(B, np.int64) if pos is None else np.asarray(pos, np.int64).reshape(-1)
    live = pos >= 0
    if states is None:
        states, word[...] = F.step_states(tables, word, start_state, start, ids, pos)
    rows = np.flatnonzero(live)
    if rows.size:
        z[rows] = F.apply(z[rows], tables, np.asarray(states)[rows])
    cv, ci = candidates_np(z)
    return live, cv, ci


def fsm_reset_np(state, rows, src):
    """pdnf_fsm_reset on arrays (in place): state = (word (B,) int64, start_state (B,), start (B,)), src = (states (R,),
    prompt lengths (R,))."""
    word, start_state, start = state
    for i, b in enumerate(np.asarray(rows).tolist()):
        if 0 <= b < word.shape[0]:
            start_state[b], start[b] = src[0][i], src[1][i]
            word[b] = F.pair(src[0][i], src[1][i])


class FsmMixin:
    # launch counter slot 52 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == FSM_SLOT:
            self.__dict__["_fsm_launches"] = self.__dict__.get("_fsm_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > FSM_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[FSM_SLOT] = self.__dict__.get("_fsm_launches", 0)
        if reset:
            self.__dict__["_fsm_launches"] = 0
        return rc

    def pdnf_fsm_chunks(self, V):
        return fsm_chunks(V)

    def pdnf_fsm_reset(self, state, start_state, start, B, rows, n_rows, s_state, s_start, stream):
        if n_rows == 0:
            return 0
        if not (state and start_state and start and rows and s_state and s_start and B > 0 and n_rows > 0):
            return -1
        R = n_rows
        fsm_reset_np((flat(state, B, np.int64), flat(start_state, B, np.int32), flat(start, B, np.int32)),
                     np.array(flat(rows, R, np.int32)),
                     (np.array(flat(s_state, R, np.int32)), np.array(flat(s_start, R, np.int32))))
        self._count(FSM_SLOT)
        return 0

    @staticmethod
    def _tables(offsets, tokens, nxt, dflt, S, E):
        return F.Tables(np.array(flat(offsets, S + 1, np.int32)), np.array(flat(tokens, E, np.int32)),
                        np.array(flat(nxt, E, np.int32)) if nxt else np.zeros(E, np.int32),
                        np.array(flat(dflt, S, np.int32)))

    def _fsm(self, logits, rs, B, V, tables, cand_v, cand_i, **how):
        Z = view(logits, (B, V), (rs, 1), np.float32)
        z = np.array(Z)
        live, cv, ci = fsm_np(z, tables, **how)
        Z[...] = z
        if cand_v:
            n = fsm_chunks(V)
            V_, I_ = flat(cand_v, B * n, np.float32).reshape(B, n), flat(cand_i, B * n, np.int32).reshape(B, n)
            V_[live], I_[live] = cv[live], ci[live]
        self._count(FSM_SLOT)
        return 0

    def pdnf_fsm_step_f32(self, logits, rs, B, V, offsets, tokens, nxt, dflt, S, E, state, start_state, start, ids, pos,
                          pos_per_row, cand_v, cand_i, stream):
        if B == 0:
            return 0
        if not (logits and offsets and tokens and nxt and dflt and state and start_state and start and ids and pos
                and B > 0 and V > 0 and S > 0 and E > 0 and rs >= V and bool(cand_v) == bool(cand_i)):
            return -1
        P = np.array(flat(pos, B if pos_per_row else 1, np.int32))
        P = P if pos_per_row else np.full(B, P[0])
        return self._fsm(logits, rs, B, V, self._tables(offsets, tokens, nxt, dflt, S, E), cand_v, cand_i,
                         word=flat(state, B, np.int64), start_state=np.array(flat(start_state, B, np.int32)),
                         start=np.array(flat(start, B, np.int32)), ids=np.array(flat(ids, B, np.int64)), pos=P)

    def pdnf_fsm_rows_f32(self, logits, rs, B, V, offsets, tokens, dflt, S, E, states, pos, cand_v, cand_i, stream):
        if B == 0:
            return 0
        if not (logits and offsets and tokens and dflt and states and B > 0 and V > 0 and S > 0 and E > 0 and rs >= V
                and bool(cand_v) == bool(cand_i)):
            return -1
        return self._fsm(logits, rs, B, V, self._tables(offsets, tokens, None, dflt, S, E), cand_v, cand_i,
                         states=np.array(flat(states, B, np.int32)),
                         pos=np.array(flat(pos, B, np.int32)) if pos else None)


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnf_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, FsmMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("Fsm" + base.__name__, (FsmMixin, base),
                                  {"__doc__": "with the entries of include/pdn_fsm.h"})
        emu.__class__ = _classes[base]
        for path in _lib.FSM_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
