"""The entries of include/pdn_dropout.h (prefix pdnd_, csrc/dropout.hip), answered with the statement of
pydynet_amd/core/fused/dropout.py; a part with a registry of its own, as tests/abi_emulator/_stopseq.py.  The host emulation
keeps no launch counter for them (slot 54 lies beyond its table).  (TEST-ONLY.)"""
import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.fused.dropout import blocks, dropout_np
from . import EmulatedLib
from ._base import flat

NOT_EMULATED = ()
_M64 = 2 ** 64 - 1


class DropoutMixin:
    def pdnd_rng_set(self, state, seed, offset, stream):
        if not state:
            return -1
        flat(state, 2, np.uint64)[:] = np.array([seed & _M64, offset & _M64], np.uint64)
        return 0

    def pdnd_rng_claim(self, state, slot, n, stream):
        if not (state and slot and n >= 0):
            return -1
        st, sl = flat(state, 2, np.uint64), flat(slot, 2, np.uint64)
        sl[:] = st
        st[1] = (int(st[1]) + blocks(n)) & _M64
        return 0

    def _dropout(self, x, res, y, n, p, slot):
        if n == 0:
            return 0
        if not (x and y and slot and n > 0 and 0 <= p < 1):
            return -1
        seed, o = (int(v) for v in flat(slot, 2, np.uint64))
        flat(y, n)[:] = dropout_np(np.array(flat(x, n)), p, seed, o, np.array(flat(res, n)) if res else None)
        return 0

    def pdnd_dropout_fwd_f32(self, x, y, n, p, slot, stream):
        return self._dropout(x, None, y, n, p, slot)

    def pdnd_dropout_add_fwd_f32(self, x, residual, out, n, p, slot, stream):
        return self._dropout(x, residual, out, n, p, slot) if residual else -1

    pdnd_dropout_bwd_f32 = pdnd_dropout_fwd_f32              # (dy, dx: the same statement)


def extend():
    """Make the installed emulator answer the pdnd_ entries as well; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, DropoutMixin):
        emu.__class__ = type("Dropout" + type(emu).__name__, (DropoutMixin, type(emu)), {})
        emu.protos.update(_lib.parse_header(_lib.DROPOUT_HEADER_PATHS[0]))
    return emu
