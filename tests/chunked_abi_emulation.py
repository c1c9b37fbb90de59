"""TEST-ONLY NumPy statements of the chunked-prefill entry points of include/pdn_hip.h (csrc/extend.hip: the KV append and
the multi-query extend attention of the mixed step), attached to the emulated library of tests/abi_emulator by the
`chunked_emulated` fixture below, with launch counter 33 next to the beam-search slot 32 (tests/beam_abi_emulation.py).
`append_np` / `extend_np` are also the float64 references of the GPU tests."""
import ctypes

import numpy as np
import pytest

from tests import beam_abi_emulation
from tests.abi_emulator import flat, view
from tests.beam_abi_emulation import beam_emulated  # noqa: F401  (fixture)

SLOTS = 34


def rotate(x, c, s):
    """Interleaved-pair RoPE of rows x (..., hd) with cos / sin rows (..., hd / 2)."""
    a, b = x[..., 0::2], x[..., 1::2]
    out = np.empty_like(x)
    out[..., 0::2], out[..., 1::2] = a * c - b * s, a * s + b * c
    return out


def run_ok(q0, n, s0, max_run, n_q, max_len):
    return 0 < n <= max_run and q0 >= 0 and q0 + n <= n_q and s0 >= 0 and s0 + n <= max_len


def append_np(qkv, cos, sin, kc, vc, runs, max_run, H, hd, max_len):
    """pdn_kv_append_rows_f32 on arrays: qkv (n_q, >= 3 D), caches (rows, max_len, D) written in place."""
    D = H * hd
    for r, (q0, n, s0, ends) in enumerate(np.asarray(runs).reshape(-1, 4).tolist()):
        if not run_ok(q0, n, s0, max_run, qkv.shape[0], max_len):
            continue
        p = np.arange(s0, s0 + n)
        k = qkv[q0:q0 + n, D:2 * D].reshape(n, H, hd)
        kc[r, s0:s0 + n] = rotate(k, cos[p][:, None, :], sin[p][:, None, :]).reshape(n, D)
        vc[r, s0:s0 + n] = qkv[q0:q0 + n, 2 * D:3 * D]
        if ends and s0 + n < max_len:
            kc[r, s0 + n] = 0
            vc[r, s0 + n] = 0


def extend_np(qkv, cos, sin, kc, vc, runs, max_run, H, hd, ns, max_len, part):
    """pdn_decode_extend_attention_f32 on arrays: part (n_q, ns, H, 4 + hd) written for the query rows of every run."""
    D = H * hd
    inv = 1.0 / np.sqrt(np.asarray(hd, qkv.dtype))
    for r, (q0, n, s0, _) in enumerate(np.asarray(runs).reshape(-1, 4).tolist()):
        if not run_ok(q0, n, s0, max_run, qkv.shape[0], max_len):
            continue
        T = s0 + n
        chunk = -(-T // ns)
        for j in range(n):
            p = s0 + j
            q = rotate(qkv[q0 + j, :D].reshape(H, hd), cos[p][None, :], sin[p][None, :])
            for sp in range(ns):
                t0, t1 = sp * chunk, min(T, sp * chunk + chunk, p + 1)
                rec = part[q0 + j, sp]
                rec[...] = 0
                if t1 <= t0:
                    rec[:, 0] = -np.inf
                    continue
                k = kc[r, t0:t1].reshape(-1, H, hd)
                v = vc[r, t0:t1].reshape(-1, H, hd)
                s = np.einsum("hd,thd->ht", q, k) * inv
                m = s.max(-1)
                e = np.exp(s - m[:, None])
                rec[:, 0], rec[:, 1] = m, e.sum(-1)
                rec[:, 4:] = np.einsum("ht,thd->hd", e, v)


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 33:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[33] = count[0]
        if reset:
            count[0] = 0
        return 0

    def pdn_decode_mixed_supported(D, H, hd, F, V, max_len):
        return int(H > 0 and hd > 0 and hd * H == D and hd % 4 == 0 and hd <= 256 and F > 0 and F % 4 == 0
                   and 0 < V <= 1 << 23 and 0 < max_len and max_len * 4 <= 60 * 1024)

    def arrays(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, n_q, H, hd, max_len):
        D = H * hd
        return (np.array(view(qkv, (n_q, 3 * D), (rs, 1), np.float32)),
                np.array(flat(cos, max_len * hd // 2)).reshape(max_len, hd // 2),
                np.array(flat(sin, max_len * hd // 2)).reshape(max_len, hd // 2),
                view(kc, (n_runs, max_len, D), (cbs, D, 1), np.float32),
                view(vc, (n_runs, max_len, D), (cbs, D, 1), np.float32),
                np.array(flat(runs, 4 * n_runs, np.int32)).reshape(n_runs, 4))

    def pdn_kv_append_rows_f32(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, max_run, n_q, H, hd, max_len, stream):
        if n_runs == 0:
            return 0
        if not (qkv and kc and vc and runs and max_run > 0 and n_q > 0 and hd % 4 == 0 and cbs >= max_len * H * hd):
            return -1
        Q, c, s, K, Vc, R = arrays(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, n_q, H, hd, max_len)
        append_np(Q, c, s, K, Vc, R, max_run, H, hd, max_len)
        count[0] += 1
        return 0

    def pdn_decode_extend_attention_f32(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, max_run, n_q, H, hd, ns, max_len,
                                        part, stream):
        if n_runs == 0:
            return 0
        if not (qkv and kc and vc and runs and part and max_run > 0 and n_q > 0 and hd % 4 == 0 and 1 <= ns <= 64):
            return -1
        Q, c, s, K, Vc, R = arrays(qkv, rs, cos, sin, kc, vc, cbs, runs, n_runs, n_q, H, hd, max_len)
        P = flat(part, n_q * ns * H * (4 + hd)).reshape(n_q, ns, H, 4 + hd)
        extend_np(Q, c, s, np.array(K), np.array(Vc), R, max_run, H, hd, ns, max_len, P)
        count[0] += 1
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def chunked_emulated(beam_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with every decode entry point up to beam search and the chunked-prefill entry points."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield beam_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return beam_abi_emulation.counters(n)
