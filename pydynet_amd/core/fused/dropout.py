"""Inverted dropout whose mask is drawn on the device from a counter-based generator, stated once in NumPy.
(One module of `pydynet_amd.core.fused`.)

This module is the contract of the kernels of csrc/dropout.hip (entries of include/pdn_dropout.h, prefix pdnd_), as
segments.py is for the segmented attention: the NumPy device (`xp is np`) runs this statement, the emulator part and the tests
compare against it, so "cpu" and the MI355X draw the same masks.  The reference's dropout (nn/modules/dropout.py) draws one
`np.random` number per element on the host; `nn.Dropout` without a generator still does exactly that.  This is an extension.

    generator   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): multipliers
                0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds
    state       two 64-bit words, `seed` and `offset` (`Generator`; in device memory on a HIP device)
    a call      over n elements CLAIMS the current offset o and leaves offset = o + ceil(n / 4)
    element i   word i % 4 of the block for counter (lo32(c), hi32(c), 0, 0), c = o + i // 4 (mod 2^64), key (lo32(seed),
                hi32(seed)); dropped iff word < floor(p * 2^32), 0 <= p < 1 (p = 0 drops nothing)
    forward     y = x * s where kept, s = float32(1) / (float32(1) - float32(p)): ONE fp32 multiply; else exactly 0
    backward    dx = dy * s where kept, else exactly 0 -- the mask comes from the same claimed (seed, o): no mask tensor exists

`dropout_add` is out = residual + dropout(x) (one fp32 multiply, one fp32 add, never contracted into an fma).

On a HIP device the claim is a launch of its own (`pdnd_rng_claim`): it copies (seed, o) into a 16-byte SLOT the tape node
owns and advances the state; forward and backward read (seed, o) from the slot, never from a launch argument.  A step
captured in a `hipnp.Graph` therefore re-runs the claim at every replay: every replay draws a fresh mask and its backward
regenerates that same mask."""
from __future__ import annotations

import numpy as np

from ...cuda import Device
from ..tensor import Tensor, _Operator
from ._common import _hip, _L, _contig, _require_f32

PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1


def philox4x32_10(counter, key):
    """The four output words (uint32 arrays) of Philox4x32-10 for `counter` = four words (ints or equal-shaped arrays) and
    `key` = two ints."""
    c = [np.asarray(v, np.uint64) & np.uint64(_M32) for v in counter]
    k0, k1 = int(key[0]) & _M32, int(key[1]) & _M32
    lo32 = np.uint64(_M32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M[0]) * c[0], np.uint64(PHILOX_M[1]) * c[2]      # (32 x 32 bits: exact in 64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo32]
        k0, k1 = (k0 + PHILOX_W[0]) & _M32, (k1 + PHILOX_W[1]) & _M32
    return [v.astype(np.uint32) for v in c]


def blocks(n):
    """Philox blocks a call over n elements claims."""
    return (int(n) + 3) // 4


def threshold(p):
    if not 0 <= p < 1 or not np.float32(p) < 1:
        raise ValueError(f"dropout probability must lie in [0, 1), got {p}")
    return int(float(p) * 4294967296.0)            # floor(p * 2^32): exact, a power of two times a double


def scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def kept(n, p, seed, offset):
    """(n,) bool: the elements a call over n elements that claimed `offset` keeps."""
    nb = blocks(n)
    c = (np.uint64(int(offset) & _M64) + np.arange(nb, dtype=np.uint64))           # (wraps mod 2^64, as the device)
    zero = np.zeros(nb, np.uint64)
    seed = int(seed) & _M64
    words = philox4x32_10((c, c >> np.uint64(32), zero, zero), (seed, seed >> 32))
    return np.stack(words, axis=1).reshape(-1)[:int(n)] >= np.uint32(threshold(p)) if n else np.zeros(0, bool)


def dropout_np(x, p, seed, offset, residual=None):
    """The forward of a call that claimed `offset` (and, with dy for x, its backward); `residual`: out = residual + it."""
    x = np.asarray(x)
    y = np.where(kept(x.size, p, seed, offset).reshape(x.shape), x * scale(p).astype(x.dtype), np.zeros((), x.dtype))
    return y if residual is None else residual + y


class Generator:
    """The state of the device-drawn dropout: `seed` and `offset`, 16 bytes on its device (two Python integers on "cpu").
    `get_state` is the only call that reads back."""

    def __init__(self, seed=0, device=None):
        self.device = device if isinstance(device, Device) else Device(device)
        if self.device.is_hip:
            with self.device:
                self._state = _hip().empty((2,), np.int64)
        self.set_state((seed, 0))

    def manual_seed(self, seed):
        self.set_state((seed, 0))
        return self

    def set_state(self, state):
        seed, offset = (int(v) & _M64 for v in state)
        if self.device.is_hip:
            with self.device:
                _L().call("pdnd_rng_set", self._state._ptr, _i64(seed), _i64(offset), _hip().stream())
        else:
            self._seed, self._offset = seed, offset

    def get_state(self):
        if self.device.is_hip:
            seed, offset = (int(v) & _M64 for v in self._state.get())
            return seed, offset
        return self._seed, self._offset

    def claim(self, n):
        """What a dropout call over n elements works from: (seed, o) on "cpu", the 16-byte slot holding them on a HIP device
        (allocated as any array of the step: inside a graph's private pool while one is captured)."""
        if not self.device.is_hip:
            got = (self._seed, self._offset)
            self._offset = (self._offset + blocks(n)) & _M64
            return got
        hp = _hip()
        slot = hp.empty((2,), np.int64)
        _L().call("pdnd_rng_claim", self._state._ptr, slot._ptr, int(n), hp.stream())
        return slot

    def __repr__(self):
        return f"Generator(device={self.device})"


def _i64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


class _Dropout(_Operator):
    """y = dropout(x) (+ residual): the node behind `dropout` / `dropout_add`."""

    def __init__(self, x, p, generator, residual=None):
        self.p, self._gen = float(p), generator
        threshold(self.p)
        if generator.device != x.device:
            raise ValueError(f"dropout: the generator lives on {generator.device}, the input on {x.device}")
        super().__init__(*((x,) if residual is None else (x, residual)))

    def forward_(self, x, r=None):
        self._claim = self._gen.claim(x.size) if x.size else None
        if self.xp is np:
            return dropout_np(x.data, self.p, *self._claim, residual=None if r is None else r.data) if x.size else x.data.copy()
        _require_f32(self, x, r)
        hp, L = _hip(), _L()
        out = hp.empty(x.shape, np.float32)
        if x.size == 0:
            return out
        xd = _contig(x.data)
        if r is None:
            L.call("pdnd_dropout_fwd_f32", xd._ptr, out._ptr, xd.size, self.p, self._claim._ptr, hp.stream())
        else:
            if r.shape != x.shape:
                raise ValueError(f"dropout_add: residual of shape {r.shape} for an input of shape {x.shape}")
            rd = _contig(r.data)
            L.call("pdnd_dropout_add_fwd_f32", xd._ptr, rd._ptr, out._ptr, xd.size, self.p, self._claim._ptr, hp.stream())
        return out

    def backward_all(self, dy):
        x = self.last[0]
        grads = [None, dy] if len(self.last) == 2 else [None]      # the residual's gradient is dy itself: no copy
        if not x.requires_grad:
            return grads
        if self.xp is np:
            grads[0] = dropout_np(dy, self.p, *self._claim) if x.size else dy
            return grads
        hp, L = _hip(), _L()
        dx = hp.empty(x.shape, np.float32)
        if x.size:
            dyc = _contig(dy)
            L.call("pdnd_dropout_bwd_f32", dyc._ptr, dx._ptr, dyc.size, self.p, self._claim._ptr, hp.stream())
        grads[0] = dx
        return grads


def dropout(x, p, generator):
    """Inverted dropout of `x` with the mask drawn from `generator` on x's device; p == 0 returns x and claims nothing."""
    if p == 0:
        return x
    return _Dropout(x, p, generator)


def dropout_add(x, residual, p, generator):
    """residual + dropout(x): the residual-dropout form, one kernel per direction."""
    if p == 0:
        return x + residual
    return _Dropout(x, p, generator, residual)
