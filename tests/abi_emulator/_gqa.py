"""The entries of include/pdn_gqattn.h (prefix pdnk_, csrc/attention_gqa.hip), answered with the statement of
pydynet_amd/core/fused/gqa.py; a part with a registry of its own, as tests/abi_emulator/_dropout.py.  The host emulation
keeps no launch counter for them (slot 55 lies beyond its table).  (TEST-ONLY.)"""
import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.fused import gqa
from . import EmulatedLib
from ._base import flat, view

NOT_EMULATED = ()
_HEAD_DIMS = (16, 24, 32, 48, 64, 96, 128)


class GqaMixin:
    def pdnk_attention_supported(self, hd, H, Hkv):
        return int(hd in _HEAD_DIMS and Hkv > 0 and H % Hkv == 0 and 2 <= H // Hkv <= 8)

    def pdnk_attention_bwd_workspace_bytes(self, B, H, Lq):
        return 4 * B * H * Lq

    @staticmethod
    def _operands(q, k, v, B, H, Hkv, Lq, Lk, hd, q_rs, q_bs, kv_rs, kv_bs, mask, sb, sh, sq, sk):
        Q = view(q, (B, Lq, H, hd), (q_bs, q_rs, hd, 1), np.float32)
        K, V = (view(p, (B, Lk, Hkv, hd), (kv_bs, kv_rs, hd, 1), np.float32) for p in (k, v))
        M = view(mask, (B, H, Lq, Lk), (sb, sh, sq, sk), np.float32) if mask else None
        return Q, K, V, M

    def pdnk_attention_fwd_f32(self, q, k, v, o, lse, B, H, Hkv, Lq, Lk, hd, q_rs, q_bs, kv_rs, kv_bs, causal, start_pos,
                               mask, sb, sh, sq, sk, stream):
        if not self.pdnk_attention_supported(hd, H, Hkv) or B * Hkv > 65535:
            return -2
        Q, K, V, M = self._operands(q, k, v, B, H, Hkv, Lq, Lk, hd, q_rs, q_bs, kv_rs, kv_bs, mask, sb, sh, sq, sk)
        out, ls, _ = gqa.forward(np.array(Q), np.array(K), np.array(V), bool(causal), start_pos, M)
        view(o, (B, Lq, H, hd), (q_bs, q_rs, hd, 1), np.float32)[...] = out
        flat(lse, B * H * Lq).reshape(B, H, Lq)[...] = ls
        return 0

    def pdnk_attention_bwd_f32(self, q, k, v, o, do, lse, dq, dk, dv, B, H, Hkv, Lq, Lk, hd, q_rs, q_bs, kv_rs, kv_bs, causal,
                               start_pos, mask, sb, sh, sq, sk, ws, wsb, stream):
        if not self.pdnk_attention_supported(hd, H, Hkv) or B * Hkv > 65535:
            return -2
        if not ws or wsb < 4 * B * H * Lq:
            return -3
        Q, K, V, M = self._operands(q, k, v, B, H, Hkv, Lq, Lk, hd, q_rs, q_bs, kv_rs, kv_bs, mask, sb, sh, sq, sk)
        Q, K, V = np.array(Q), np.array(K), np.array(V)
        DO = np.array(view(do, (B, Lq, H, hd), (q_bs, q_rs, hd, 1), np.float32))
        _, _, p = gqa.forward(Q, K, V, bool(causal), start_pos, M)
        gq, gk, gv = gqa.backward(Q, K, V, p, DO)
        view(dq, (B, Lq, H, hd), (q_bs, q_rs, hd, 1), np.float32)[...] = gq
        view(dk, (B, Lk, Hkv, hd), (kv_bs, kv_rs, hd, 1), np.float32)[...] = gk
        view(dv, (B, Lk, Hkv, hd), (kv_bs, kv_rs, hd, 1), np.float32)[...] = gv
        return 0


def extend():
    """Make the installed emulator answer the pdnk_ entries as well; nothing happens on the real library."""
    emu = _lib._LIB
    if isinstance(emu, EmulatedLib) and not isinstance(emu, GqaMixin):
        emu.__class__ = type("Gqa" + type(emu).__name__, (GqaMixin, type(emu)), {})
        emu.protos.update(_lib.parse_header(_lib.GQA_HEADER_PATHS[0]))
    return emu
