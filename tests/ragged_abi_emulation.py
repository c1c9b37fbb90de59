"""TEST-ONLY NumPy statements of the ragged-decode entry points of include/pdn_hip.h (the *_rows_f32 entries of
csrc/decode.hip, decode_block.hip, sample.hip and attention.hip), attached to the emulated library of tests/abi_emulator
by the `ragged_emulated` fixture below, with launch counter 29 next to the sampling slot 28
(tests/sampling_abi_emulation.py).  Each per-row entry runs the emulator's own scalar statement once per row, at that
row's position (a stopped row, pos < 0: at position 0, its cache slot put back afterwards)."""
import ctypes

import numpy as np
import pytest

from pydynet_amd.llm import sampling
from tests import sampling_abi_emulation
from tests.abi_emulator import flat, view
from tests.sampling_abi_emulation import read_params, sampling_emulated  # noqa: F401  (fixture)

SLOTS = 30


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 29:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[29] = count[0]
        if reset:
            count[0] = 0
        return 0

    def per_row(B, pos, kc, vc, cbs, D, run):
        """run(b, pos_ptr) for every row with a one-element position buffer; a stopped row's slot 0 is put back."""
        p = np.array(flat(pos, B, np.int32))
        for b in range(B):
            one = np.array([max(int(p[b]), 0)], np.int32)
            kslot, vslot = kc + 4 * b * cbs, vc + 4 * b * cbs
            keep = (np.array(flat(kslot, D)), np.array(flat(vslot, D))) if p[b] < 0 else None
            rc = run(b, one.ctypes.data)
            if keep is not None:
                flat(kslot, D)[...], flat(vslot, D)[...] = keep
            if rc:
                return rc
        count[0] += 1
        return 0

    def off(ptr, floats):
        return ptr + 4 * floats if ptr else ptr

    def pdn_decode_block_rows_f32(base, base_rs, parts, n_parts, parts_rs, x_out, x_out_rs, norm_w, eps, Wqkv, w_rs, w_bs,
                                  cos, sin, kc, vc, cbs, pos, max_len, Wo, wo_rs, recs, B, H, hd, NS, stream):
        D = H * hd
        if B > 8:
            return -1
        rr = (NS + 1) * H * (4 + D)
        return per_row(B, pos, kc, vc, cbs, D, lambda b, p: emu.pdn_decode_block_f32(
            off(base, b * base_rs), base_rs, off(parts, b * parts_rs), n_parts, parts_rs, off(x_out, b * x_out_rs),
            x_out_rs, norm_w, eps, Wqkv, w_rs, w_bs, cos, sin, off(kc, b * cbs), off(vc, b * cbs), cbs, p, max_len, Wo,
            wo_rs, off(recs, b * rr), 1, H, hd, NS, stream))

    def pdn_decode_attention_rows_f32(qkv, rs, cos, sin, kc, vc, parts, B, H, hd, NS, cbs, pos, max_len, stream):
        rr = NS * H * (4 + hd)
        return per_row(B, pos, kc, vc, cbs, H * hd, lambda b, p: emu.pdn_decode_attention_f32(
            off(qkv, b * rs), rs, cos, sin, off(kc, b * cbs), off(vc, b * cbs), off(parts, b * rr), 1, H, hd, NS, cbs,
            p, max_len, stream))

    def pdn_decode_attention_oproj_rows_f32(qkv, rs, cos, sin, kc, vc, Wo, wo_rs, recs, B, H, hd, NS, cbs, pos, max_len,
                                            stream):
        D = H * hd
        rr = NS * H * (4 + D)
        return per_row(B, pos, kc, vc, cbs, D, lambda b, p: emu.pdn_decode_attention_oproj_f32(
            off(qkv, b * rs), rs, cos, sin, off(kc, b * cbs), off(vc, b * cbs), Wo, wo_rs, off(recs, b * rr), 1, H, hd,
            NS, cbs, p, max_len, stream))

    def tick(B, pos, step, stop, hist, emb, emb_rs, D, x_next, pick):
        """The per-row tick around pick(b, position) -> token."""
        P = flat(pos, B, np.int32)
        s = int(flat(step, 1, np.int32)[0])
        hrow = flat(int(flat(hist, 1, np.int64)[0]) + 8 * s * B, B, np.int64) if hist else None
        for b in range(B):
            p = int(P[b])
            if p < 0:
                if hrow is not None:
                    hrow[b] = -1
                continue
            tok = int(pick(b, p))
            if hrow is not None:
                hrow[b] = tok
            if emb:
                flat(x_next, B * D).reshape(B, D)[b] = flat(emb + 4 * tok * emb_rs, D)
            if stop:
                mask = np.array(flat(stop, tok // 32 + 1, np.int32)).view(np.uint32)
            P[b] = -1 if stop and (mask[tok >> 5] >> np.uint32(tok & 31)) & 1 else p + 1
        flat(step, 1, np.int32)[0] = s + 1
        count[0] += 1
        return 0

    def pdn_decode_pick_tick_rows_f32(vals, args, B, n, ids, pos, step, stop, hist, emb, emb_rs, D, x_next, stream):
        v = np.array(flat(vals, B * n).reshape(B, n))
        a = np.array(flat(args, B * n, np.int32).reshape(B, n))

        def pick(b, p):
            tok = a[b][v[b] == v[b].max()].min()
            flat(ids, B, np.int64)[b] = tok
            return tok
        return tick(B, pos, step, stop, hist, emb, emb_rs, D, x_next, pick)

    def pdn_decode_sample_tick_rows_f32(logits, rs, B, V, params, ids, pos, step, stop, hist, emb, emb_rs, D, x_next,
                                        stream):
        T, k, p_, seed = read_params(params)
        z = np.array(view(logits, (B, V), (rs, 1), np.float32))

        def pick(b, p):
            tok = sampling.sample_rows_np(z[b:b + 1], p, T, k, p_, seed, rows=[b])[0] if T > 0 else z[b].argmax()
            flat(ids, B, np.int64)[b] = tok
            return tok
        rc = tick(B, pos, step, stop, hist, emb, emb_rs, D, x_next, pick)
        scratch = np.zeros(1, np.int64)                  # (counter 28 as well, as the real tick: one launch of the sampler)
        emu.pdn_sample_rows_f32(logits, rs, 1, V, params, 0, scratch.ctypes.data, stream)
        return rc

    def pdn_attention_decode_rows_f32(q, kc, vc, o, B, H, lens, max_T, hd, cbs, stream):
        D = H * hd
        T = np.clip(np.array(flat(lens, B, np.int32)), 1, max_T)
        for b in range(B):
            emu.pdn_attention_decode_f32(off(q, b * D), off(kc, b * cbs), off(vc, b * cbs), off(o, b * D), 1, H, int(T[b]),
                                         hd, cbs, stream)
        count[0] += 1
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def ragged_emulated(sampling_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with the CLIP, sampling and ragged-decode entry points attached."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield sampling_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return sampling_abi_emulation.counters(n)
