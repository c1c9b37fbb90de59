"""TEST-ONLY NumPy statements of the continuous-batching entry points of include/pdn_hip.h (Llama.serve: the slot ticks of
csrc/decode.hip and sample.hip, pdn_kv_store_slots_f32 of csrc/serve.hip), attached to the emulated library of
tests/abi_emulator by the `serve_emulated` fixture below, with launch counter 30 next to the ragged slot 29
(tests/ragged_abi_emulation.py)."""
import ctypes

import numpy as np
import pytest

from pydynet_amd.llm import sampling
from tests import ragged_abi_emulation
from tests.abi_emulator import flat, view
from tests.ragged_abi_emulation import ragged_emulated  # noqa: F401  (fixture)
from tests.sampling_abi_emulation import read_params

SLOTS = 31


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 30:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[30] = count[0]
        if reset:
            count[0] = 0
        return 0

    def tick(B, pos, step, left, ring, stop, hist, emb, emb_rs, D, x_next, pick):
        """The slot tick around pick(b, position) -> token: a history ring, a budget per row."""
        P, Lf = flat(pos, B, np.int32), flat(left, B, np.int32)
        s = int(flat(step, 1, np.int32)[0])
        hrow = flat(int(flat(hist, 1, np.int64)[0]) + 8 * (s % ring) * B, B, np.int64) if hist else None
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
            hit = False
            if stop:
                mask = np.array(flat(stop, tok // 32 + 1, np.int32)).view(np.uint32)
                hit = bool((mask[tok >> 5] >> np.uint32(tok & 31)) & 1)
            Lf[b] -= 1
            P[b] = -1 if hit or Lf[b] <= 0 else p + 1
        flat(step, 1, np.int32)[0] = s + 1
        count[0] += 1
        return 0

    def pdn_decode_pick_tick_slots_f32(vals, args, B, n, ids, pos, step, req, left, ring, stop, hist, emb, emb_rs, D,
                                       x_next, stream):
        if B == 0:
            return 0
        if not (vals and args and ids and pos and step and left and ring > 0):
            return -1
        v = np.array(flat(vals, B * n).reshape(B, n))
        a = np.array(flat(args, B * n, np.int32).reshape(B, n))

        def pick(b, p):
            tok = a[b][v[b] == v[b].max()].min()
            flat(ids, B, np.int64)[b] = tok
            return tok
        return tick(B, pos, step, left, ring, stop, hist, emb, emb_rs, D, x_next, pick)

    def pdn_decode_sample_tick_slots_f32(logits, rs, B, V, params, ids, pos, step, req, left, ring, stop, hist, emb,
                                         emb_rs, D, x_next, stream):
        if B == 0:
            return 0
        if not (logits and params and ids and pos and step and req and left and ring > 0):
            return -1
        T, k, p_, seed = read_params(params)
        z = np.array(view(logits, (B, V), (rs, 1), np.float32))
        R = np.array(flat(req, B, np.int32))

        def pick(b, p):
            tok = sampling.sample_rows_np(z[b:b + 1], p, T, k, p_, seed, rows=[int(R[b])])[0] if T > 0 else z[b].argmax()
            flat(ids, B, np.int64)[b] = tok
            return tok
        rc = tick(B, pos, step, left, ring, stop, hist, emb, emb_rs, D, x_next, pick)
        scratch = np.zeros(1, np.int64)                  # (counter 28 as well, as the real tick: one launch of the sampler)
        emu.pdn_sample_rows_f32(logits, rs, 1, V, params, 0, scratch.ctypes.data, stream)
        return rc

    def pdn_kv_store_slots_f32(src, src_bs, dst, dst_bs, n_tensors, n_inputs, Ls, D, slots, lens, start, n_rows,
                               max_len, stream):
        if n_tensors == 0 or n_inputs == 0 or Ls == 0:
            return 0
        if not (src and dst and slots and lens and D > 0 and src_bs >= 0 and dst_bs >= max_len * D):
            return -1
        S = flat(src, n_tensors, np.int64)
        Dt = flat(dst, n_tensors, np.int64)
        sl, ln = flat(slots, n_inputs, np.int32), flat(lens, n_inputs, np.int32)
        s0 = flat(start, n_inputs, np.int32) if start else np.zeros(n_inputs, np.int32)
        for j in range(n_tensors):
            for i in range(n_inputs):
                row, a = int(sl[i]), int(s0[i])
                n = min(int(ln[i]), Ls, max_len - a)
                if row < 0 or row >= n_rows or a < 0 or n <= 0:
                    continue
                out = flat(int(Dt[j]) + 4 * (row * dst_bs + a * D), n * D)
                out[...] = flat(int(S[j]) + 4 * i * src_bs, n * D)
        count[0] += 1
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def serve_emulated(ragged_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with the CLIP, sampling, ragged-decode and continuous-batching entry points attached."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield ragged_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return ragged_abi_emulation.counters(n)
