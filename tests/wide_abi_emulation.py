"""TEST-ONLY NumPy statements of the wide-decode entry points of include/pdn_hip.h (csrc/decode_wide.hip: the MFMA
product with its load modes and epilogues, the workgroup-per-row ticks), attached to the emulated library of
tests/abi_emulator by the `wide_emulated` fixture below, with launch counter 31 next to the continuous-batching slot 30
(tests/serve_abi_emulation.py).  The wide ticks run the emulator's own ragged / slot ticks (which count in 28 - 30 as the
real ones do) and count in 31."""
import ctypes

import numpy as np
import pytest

from tests import serve_abi_emulation
from tests.abi_emulator import flat, view
from tests.serve_abi_emulation import serve_emulated  # noqa: F401  (fixture)

SLOTS = 32
TN = 32                                   # columns per candidate block (csrc/decode_wide.hip: WD_TN)


def gemm_np(X, mode, norm_w, eps, ns, hd, W, bias, K):
    """The product of pdn_decode_wide_gemm_f32 before its epilogue: A(X) @ W + bias, float32 (X: the input rows as
    the entry reads them; W: (K, N) float32)."""
    B = X.shape[0]
    if mode == 3:
        H = K // hd
        R = X[:, :ns * H * (4 + hd)].reshape(B, ns, H, 4 + hd)
        m, l, o = R[..., 0], R[..., 1], R[..., 4:]
        m = np.where(l > 0, m, -np.inf)
        w = np.where(l > 0, np.exp(m - m.max(1, keepdims=True)), 0).astype(np.float32)
        a = ((w[..., None] * o).sum(1) / (w * l).sum(1)[..., None]).reshape(B, K)
    elif mode == 2:
        g, u = X[:, :K], X[:, K:2 * K]
        a = g / (np.float32(1) + np.exp(-g)) * u
    elif mode == 1:
        a = X[:, :K] / np.sqrt((X[:, :K] * X[:, :K]).mean(-1, keepdims=True) + np.float32(eps)) * norm_w
    else:
        a = X[:, :K]
    out = (a.astype(np.float32) @ W).astype(np.float32)
    return out + bias if bias is not None else out


def candidates(out):
    """First maximum and its column per row and 32-column block (the epi 2 candidates)."""
    B, N = out.shape
    nb = -(-N // TN)
    v, a = np.empty((B, nb), np.float32), np.empty((B, nb), np.int32)
    for j in range(nb):
        seg = out[:, j * TN:(j + 1) * TN]
        v[:, j], a[:, j] = seg.max(-1), j * TN + seg.argmax(-1)
    return v, a


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 31:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[31] = count[0]
        if reset:
            count[0] = 0
        return 0

    def pdn_decode_wide_supported(B, D, H, hd, F, V, max_len):
        return int(9 <= B <= 256 and H > 0 and hd * H == D and hd % 4 == 0 and hd <= 256 and D % 4 == 0 and F > 0
                   and F % 4 == 0 and 0 < V <= 1 << 23 and 0 < max_len and max_len * 4 <= 60 * 1024)

    def pdn_decode_wide_blocks(N):
        return -(-N // TN) if N > 0 else 0

    def pdn_decode_wide_work_floats(B, K, N):
        return 0                          # (the emulated product needs no workspace)

    def pdn_decode_wide_gemm_f32(x, x_rs, mode, norm_w, eps, ns, hd, W, w_rs, blk_cols, w_bs, bias, y, y_rs, epi, cand_v,
                                 cand_i, pos, B, K, N, work, stream):
        if B == 0 or N == 0:
            return 0
        if not (x and W and y and 0 < B <= 256 and K % 4 == 0 and N % blk_cols == 0 and 0 <= mode <= 3 and 0 <= epi <= 2):
            return -1
        width = {0: K, 1: K, 2: 2 * K, 3: ns * (K // max(hd, 1)) * (4 + hd)}[mode]
        X = np.array(view(x, (B, width), (x_rs, 1), np.float32))
        nb = N // blk_cols
        Wm = np.concatenate([np.array(view(W + 4 * j * w_bs, (K, blk_cols), (w_rs, 1), np.float32)) for j in range(nb)],
                            axis=1)
        out = gemm_np(X, mode, flat(norm_w, K) if norm_w else None, eps, ns, hd, Wm,
                      np.array(flat(bias, N)) if bias else None, K)
        live = np.array(flat(pos, B, np.int32)) >= 0 if pos else np.ones(B, bool)
        Y = view(y, (B, N), (y_rs, 1), np.float32)
        Y[live] = (Y[live] + out[live]) if epi == 1 else out[live]
        if epi == 2:
            v, a = candidates(out)
            nbk = pdn_decode_wide_blocks(N)
            flat(cand_v, B * nbk).reshape(B, nbk)[live] = v[live]
            flat(cand_i, B * nbk, np.int32).reshape(B, nbk)[live] = a[live]
        count[0] += 1
        return 0

    def counted(rc):
        count[0] += 1
        return rc

    def pdn_decode_wide_pick_tick_rows_f32(vals, args, B, n, ids, pos, step, arrive, stop, hist, emb, emb_rs, D, x_next,
                                           stream):
        return counted(emu.pdn_decode_pick_tick_rows_f32(vals, args, B, n, ids, pos, step, stop, hist, emb, emb_rs, D,
                                                         x_next, stream))

    def pdn_decode_wide_pick_tick_slots_f32(vals, args, B, n, ids, pos, step, arrive, req, left, ring, stop, hist, emb,
                                            emb_rs, D, x_next, stream):
        return counted(emu.pdn_decode_pick_tick_slots_f32(vals, args, B, n, ids, pos, step, req, left, ring, stop, hist,
                                                          emb, emb_rs, D, x_next, stream))

    def pdn_decode_wide_sample_tick_rows_f32(logits, rs, B, V, params, ids, pos, step, arrive, stop, hist, emb, emb_rs,
                                             D, x_next, stream):
        return counted(emu.pdn_decode_sample_tick_rows_f32(logits, rs, B, V, params, ids, pos, step, stop, hist, emb,
                                                           emb_rs, D, x_next, stream))

    def pdn_decode_wide_sample_tick_slots_f32(logits, rs, B, V, params, ids, pos, step, arrive, req, left, ring, stop,
                                              hist, emb, emb_rs, D, x_next, stream):
        return counted(emu.pdn_decode_sample_tick_slots_f32(logits, rs, B, V, params, ids, pos, step, req, left, ring,
                                                            stop, hist, emb, emb_rs, D, x_next, stream))

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def wide_emulated(serve_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with the CLIP, sampling, ragged, continuous-batching and wide-decode entry points attached."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield serve_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return serve_abi_emulation.counters(n)
