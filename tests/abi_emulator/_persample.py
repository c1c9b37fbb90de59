"""Sampling parameters per row (csrc/sample.hip, decode_wide.hip, speculative.hip): the entries of include/pdn_persample.h
(prefix pdnq_).  As for the pdnx_, pdnl_, pdns_, pdnr_, pdnz_ and pdne_ entries (_optim.py, _loss.py, _segattn.py, _rowloss.py,
_smoothloss.py, _logitedit.py) the core header's registry is closed to them, so this part carries its own: `PerSampleMixin`,
its `NOT_EMULATED` and `extend()`.  tests/test_persample_abi_cpu.py holds header, exports and this part equal.  Every entry
states the contract through the product's module, pydynet_amd/llm/sampling.py; `draw_np` and `margin` are also the references
of the GPU tests.
(TEST-ONLY host emulation: see tests/abi_emulator/__init__.py.)"""
import ctypes

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.llm import sampling
from . import EmulatedLib
from . import _sampling
from ._base import flat, view

NOT_EMULATED = ()
PERSAMPLE_SLOT = 49                              # PDN_CNT_PERSAMPLE of csrc/common.h


def read_block(words):
    """(temperature, top_k, top_p, seed, min_p) of one 24-byte parameter block given as three int64 words."""
    raw = np.ascontiguousarray(words, np.int64).view(np.uint8)
    return (float(raw[0:4].view(np.float32)[0]), int(raw[4:8].view(np.int32)[0]), float(raw[8:12].view(np.float32)[0]),
            int(raw[16:24].view(np.uint64)[0]), float(raw[12:16].view(np.float32)[0]))


def draw_np(z, block, t, b):
    """One row's token under its block (three int64 words) with counter (t, b): the statement of llm/sampling.py."""
    T, k, p, seed, m = read_block(block)
    if not T > 0:
        return int(np.asarray(z).argmax())
    return int(sampling.sample_rows_np(np.asarray(z)[None], int(t), T, k, p, seed, rows=[int(b)], min_p=m)[0])


def margin(z, t, b, temperature, top_k, top_p, seed, min_p=0.0):
    """`_sampling.margin` extended by min_p: the float64 distance of the nearest weight exp((z_i - max z) / T) of a token
    kept by steps 1-3 to min_p, and of the CDF steps of the min_p-truncated distribution to u."""
    out = _sampling.margin(z, t, b, temperature, top_k, top_p, seed)
    if min_p > 0.0:
        z = np.asarray(z, np.float64)
        kept, _ = sampling.kept_mask(z, top_k, top_p, temperature)
        out = min(out, float(np.abs(np.exp((z[kept] - z.max()) / temperature) - min_p).min()))
        _, p = sampling.kept_mask(z, top_k, top_p, temperature, min_p)
        out = min(out, float(np.abs(np.cumsum(p)[p > 0] - sampling.uniforms(t, [b], seed)[0]).min()))
    return out


def _table_pick(logits, rs, B, V, params, ids, per=1):
    """pick(r, position) -> row r's draw under block r // per, on the random stream ids[r]."""
    blocks = np.array(flat(params, 3 * (-(-B // per)), np.int64)).reshape(-1, 3)
    z = np.array(view(logits, (B, V), (rs, 1), np.float32))
    return lambda r, p: draw_np(z[r], blocks[r // per], p, ids[r])


class PerSampleMixin:
    # launch counter slot 49 lies beyond the emulator's own table (_gemm.SLOTS): kept here, reported and reset with the others
    def _count(self, slot):
        if slot == PERSAMPLE_SLOT:
            self.__dict__["_persample_launches"] = self.__dict__.get("_persample_launches", 0) + 1
        else:
            super()._count(slot)

    def pdn_kernel_counters(self, out, n, reset):
        rc = super().pdn_kernel_counters(out, n, reset)
        if out and int(n) > PERSAMPLE_SLOT:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[PERSAMPLE_SLOT] = self.__dict__.get("_persample_launches", 0)
        if reset:
            self.__dict__["_persample_launches"] = 0
        return rc

    def pdnq_sample_rows_f32(self, logits, rs, B, V, params, pos, req, out, stream):
        if B == 0:
            return 0
        if not (logits and params and pos and out and 0 < B <= 65535 and 0 < V <= 1 << 23 and rs >= V):
            return -1
        P = np.array(flat(pos, B, np.int32))
        ids = np.array(flat(req, B, np.int32)) if req else np.arange(B)
        pick, O = _table_pick(logits, rs, B, V, params, ids), flat(out, B, np.int64)
        for b in np.flatnonzero(P >= 0):
            O[b] = pick(int(b), int(P[b]))
        self._count(28)
        self._count(PERSAMPLE_SLOT)
        return 0

    # the ticks: DecodeRowsMixin._tick around the per-row pick; counted as the shared forms of _decode_rows.py count
    def _table_tick(self, logits, rs, B, V, params, ids_of, *tick, **slots):
        rc = self._tick(_table_pick(logits, rs, B, V, params, ids_of), B, *tick, **slots)
        self._count(28)
        self._count(PERSAMPLE_SLOT)
        return rc

    def pdnq_decode_sample_tick_rows_f32(self, logits, rs, B, V, params, ids, pos, step, stop, hist, emb, emb_rs, D, x_next,
                                         stream):
        if B == 0:
            return 0
        if not (logits and params and ids and pos and step and B > 0 and 0 < V <= 1 << 23 and rs >= V):
            return -1
        return self._table_tick(logits, rs, B, V, params, range(B), ids, pos, step, stop, hist, emb, emb_rs, D, x_next)

    def pdnq_decode_sample_tick_slots_f32(self, logits, rs, B, V, params, ids, pos, step, req, left, ring, stop, hist, emb,
                                          emb_rs, D, x_next, stream):
        if B == 0:
            return 0
        if not (logits and params and ids and pos and step and req and left and ring > 0 and B > 0 and rs >= V > 0):
            return -1
        return self._table_tick(logits, rs, B, V, params, np.array(flat(req, B, np.int32)), ids, pos, step, stop, hist, emb,
                                emb_rs, D, x_next, left=left, ring=ring)

    def pdnq_decode_wide_sample_tick_rows_f32(self, logits, rs, B, V, params, ids, pos, step, arrive, stop, hist, emb,
                                              emb_rs, D, x_next, stream):
        return self._counted_wide(self.pdnq_decode_sample_tick_rows_f32(logits, rs, B, V, params, ids, pos, step, stop,
                                                                        hist, emb, emb_rs, D, x_next, stream))

    def pdnq_decode_wide_sample_tick_slots_f32(self, logits, rs, B, V, params, ids, pos, step, arrive, req, left, ring,
                                               stop, hist, emb, emb_rs, D, x_next, stream):
        return self._counted_wide(self.pdnq_decode_sample_tick_slots_f32(logits, rs, B, V, params, ids, pos, step, req,
                                                                         left, ring, stop, hist, emb, emb_rs, D, x_next,
                                                                         stream))

    def pdnq_spec_verify_sample_tick_f32(self, logits, rs, V, params, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left,
                                         stop, step, mailbox, stream):
        if not (logits and params and V > 0 and rs >= V and tokens and qpos and picks and hist and step and B > 0):
            return -1
        R = B * (k + 1)
        pick = _table_pick(logits, rs, R, V, params, np.arange(R) // (k + 1), per=k + 1)
        rc = self._spec_tick(pick, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step, mailbox, V)
        self._count(PERSAMPLE_SLOT)
        return rc


_classes = {}


def extend():
    """Make the installed emulator (tests/abi_emulator.install, the `emulated_hip` fixture) answer the pdnq_ entries as well,
    whatever other parts it was extended by before; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, PerSampleMixin):
        base = type(emu)
        if base not in _classes:
            _classes[base] = type("PerSample" + base.__name__, (PerSampleMixin, base),
                                  {"__doc__": "with the entries of include/pdn_persample.h"})
        emu.__class__ = _classes[base]
        for path in _lib.PERSAMPLE_HEADER_PATHS:
            emu.protos.update(_lib.parse_header(path))
    return emu
