"""TEST-ONLY NumPy statements of the sampling entry points of include/pdn_hip.h (csrc/sample.hip), attached to the emulated
library of tests/abi_emulator by the `sampling_emulated` fixture below: pdn_sample_rows_f32, pdn_decode_sample_tick_f32 and
launch counter 28 next to the CLIP slots 24-27 (tests/clip_abi_emulation.py).  Both run the contract of
pydynet_amd/llm/sampling.py on the fp32 rows; `margin` is the float64 distance of a draw from a decision boundary."""
import ctypes

import numpy as np
import pytest

from pydynet_amd.llm import sampling
from tests import clip_abi_emulation
from tests.abi_emulator import flat, view
from tests.clip_abi_emulation import clip_emulated  # noqa: F401  (fixture)

SLOTS = 29


def read_params(ptr):
    raw = np.array(flat(ptr, 3, np.int64)).view(np.uint8)
    return (float(raw[0:4].view(np.float32)[0]), int(raw[4:8].view(np.int32)[0]), float(raw[8:12].view(np.float32)[0]),
            int(raw[16:24].view(np.uint64)[0]))


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 28:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[28] = count[0]
        if reset:
            count[0] = 0
        return 0

    def pdn_sample_rows_f32(logits, rs, B, V, params, t, out, stream):
        if B == 0:
            return 0
        T, k, p, seed = read_params(params)
        z = np.array(view(logits, (B, V), (rs, 1), np.float32))
        flat(out, B, np.int64)[...] = sampling.sample_rows_np(z, int(t), T, k, p, seed) if T > 0 else z.argmax(-1)
        count[0] += 1
        return 0

    def pdn_decode_sample_tick_f32(logits, rs, B, V, params, ids, pos, hist, emb, emb_rs, D, x_next, stream):
        if B == 0:
            return 0
        p = int(flat(pos, 1, np.int32)[0]) if pos else 0
        pdn_sample_rows_f32(logits, rs, B, V, params, p, ids, stream)
        tok = np.array(flat(ids, B, np.int64))
        if hist:
            flat(int(flat(hist, 1, np.int64)[0]) + 8 * p * B, B, np.int64)[...] = tok
        if emb:
            for b in range(B):
                flat(x_next, B * D).reshape(B, D)[b] = flat(emb + 4 * int(tok[b]) * emb_rs, D)
        if pos:
            flat(pos, 1, np.int32)[0] += 1
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def sampling_emulated(clip_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with the CLIP entry points and the sampling entry points attached."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield clip_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return clip_abi_emulation.counters(n)


def margin(z, t, b, temperature, top_k, top_p, seed):
    """float64 distance of row b's draw from the nearest decision boundary, relative to the total mass 1: the CDF steps
    against u, the top-p mass of the value groups against top_p, the top-k gap at the k-th value (relative to its size)."""
    z = np.asarray(z, np.float64)
    V = z.shape[0]
    out = np.inf
    if 0 < top_k < V:
        s = np.sort(z)[::-1]
        out = min(out, (s[top_k - 1] - s[top_k]) / max(1.0, abs(s[top_k - 1])) if s[top_k - 1] != s[top_k] else np.inf)
    if top_p < 1.0:
        kept = np.ones(V, bool) if not 0 < top_k < V else z >= np.partition(z, V - top_k)[V - top_k]
        w = np.where(kept, np.exp((z - z.max()) / temperature), 0.0)
        vals, grp = np.unique(z[kept], return_inverse=True)
        cum = np.cumsum(np.bincount(grp.reshape(-1), weights=(w / w.sum())[kept], minlength=vals.size)[::-1])
        out = min(out, float(np.abs(cum - top_p).min()))
    _, p = sampling.kept_mask(z, top_k, top_p, temperature)
    u = sampling.uniforms(t, [b], seed)[0]
    out = min(out, float(np.abs(np.cumsum(p)[p > 0] - u).min()))
    return out
