"""TEST-ONLY NumPy statements of the speculative-decoding entry points of include/pdn_hip.h (csrc/speculative.hip: the draft
kernel and the two verify ticks), attached to the emulated library of tests/abi_emulator by the `speculative_emulated`
fixture below, with launch counter 34 next to the chunked-prefill slot 33 (tests/chunked_abi_emulation.py).
`draft_np` / `settle_np` are also the references of the GPU tests; both follow pydynet_amd/llm/speculative.py."""
import ctypes

import numpy as np
import pytest

from pydynet_amd.llm import sampling, speculative
from tests import chunked_abi_emulation
from tests.abi_emulator import flat
from tests.beam_abi_emulation import beam_emulated  # noqa: F401  (fixture)
from tests.chunked_abi_emulation import chunked_emulated  # noqa: F401  (fixture)
from tests.sampling_abi_emulation import read_params

SLOTS = 35


def draft_np(hist, hlen, pos, left, k):
    """pdn_spec_draft_rows on arrays: (tokens (B (k + 1),) int64, qpos (B (k + 1),) int32, runs (B, 4) int32)."""
    B, K1 = len(pos), k + 1
    tok, qpos, runs = np.zeros(B * K1, np.int64), np.full(B * K1, -1, np.int32), np.zeros((B, 4), np.int32)
    for b in range(B):
        runs[b, 0] = b * K1
        if pos[b] < 0 or hlen[b] < 1:
            continue
        h = np.asarray(hist[b][:hlen[b]], np.int64)
        d = speculative.draft(h, k, left[b])
        tok[b * K1] = h[-1]
        tok[b * K1 + 1:b * K1 + 1 + d.size] = d
        qpos[b * K1:b * K1 + 1 + d.size] = pos[b] + np.arange(d.size + 1)
        runs[b] = (b * K1, d.size + 1, pos[b], 0)
    return tok, qpos, runs


def settle_np(tok, qpos, picks, k, hist, hlen, pos, left, stops):
    """The accept part of both ticks on arrays (hist / hlen / pos / left updated in place): the (B, k + 4) mailbox slot."""
    B, K1 = len(pos), k + 1
    out = np.full((B, k + 4), -1, np.int64)
    out[:, :3] = 0
    for b in range(B):
        if pos[b] < 0:
            continue
        d = 0
        while d < k and qpos[b * K1 + d + 1] >= 0:
            d += 1
        fed, got = tok[b * K1:b * K1 + d + 1], picks[b * K1:b * K1 + d + 1]
        y, a, hit = speculative.accept(fed, got, left[b], stops)
        c = y.size
        hist[b][hlen[b]:hlen[b] + c] = y
        hlen[b] += c
        left[b] -= c
        pos[b] = -1 if (hit or left[b] <= 0) else pos[b] + c
        out[b, :3] = (c, d, min(a, c))
        out[b, 3:3 + c] = y
    return out


def _stops(mask_ptr, V):
    if not mask_ptr:
        return np.zeros(0, np.int64)
    m = np.array(flat(mask_ptr, -(-V // 32), np.int32)).view(np.uint32)
    bits = (m[:, None] >> np.arange(32, dtype=np.uint32)) & 1
    return np.flatnonzero(bits.reshape(-1))


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 34:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[34] = count[0]
        if reset:
            count[0] = 0
        return 0

    def pdn_spec_draft_rows(hist, hs, hlen, pos, left, B, k, tokens, qpos, runs, stream):
        if not (hist and hlen and pos and left and tokens and qpos and runs and B > 0 and 0 <= k <= 16 and hs > 0):
            return -1
        H = flat(hist, B * hs, np.int32).reshape(B, hs)
        t, q, r = draft_np(H, np.array(flat(hlen, B, np.int32)), np.array(flat(pos, B, np.int32)),
                           np.array(flat(left, B, np.int32)), k)
        flat(tokens, B * (k + 1), np.int64)[...] = t
        flat(qpos, B * (k + 1), np.int32)[...] = q
        flat(runs, 4 * B, np.int32)[...] = r.reshape(-1)
        count[0] += 1
        return 0

    def tick(picks_of, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step, mailbox, V):
        R = B * (k + 1)
        q = np.array(flat(qpos, R, np.int32))
        P = flat(picks, R, np.int64)
        for r in np.flatnonzero(q >= 0):
            P[r] = picks_of(int(r), int(q[r]))
        H, HL, PS, LF = (flat(hist, B * hs, np.int32).reshape(B, hs), flat(hlen, B, np.int32), flat(pos, B, np.int32),
                         flat(left, B, np.int32))
        hl, ps, lf = (np.array(a, np.int64) for a in (HL, PS, LF))
        V = int(V or np.array(P)[q >= 0].max(initial=0) + 1)        # (the pick tick: bits up to the largest pick)
        out = settle_np(np.array(flat(tokens, R, np.int64)), q, np.array(P), k, H, hl, ps, lf, _stops(stop, V))
        HL[...], PS[...], LF[...] = hl, ps, lf
        s = flat(step, 1, np.int32)
        mb = int(flat(mailbox, 1, np.int64)[0]) if mailbox else 0
        if mb:
            flat(mb + 8 * int(s[0]) * B * (k + 4), B * (k + 4), np.int64)[...] = out.reshape(-1)
        s[0] += 1
        count[0] += 1
        return 0

    def pdn_spec_verify_pick_tick_f32(vals, args, n, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step,
                                      mailbox, stream):
        if not (vals and args and n > 0 and tokens and qpos and picks and hist and step and B > 0 and 0 <= k <= 16):
            return -1
        Vv = flat(vals, B * (k + 1) * n, np.float32).reshape(-1, n)
        Ai = flat(args, B * (k + 1) * n, np.int32).reshape(-1, n)

        def pick(r, p):
            best = Vv[r].max()
            return int(Ai[r][Vv[r] == best].min())
        return tick(pick, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step, mailbox, 0)

    def pdn_spec_verify_sample_tick_f32(logits, rs, V, params, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left,
                                        stop, step, mailbox, stream):
        if not (logits and params and V > 0 and rs >= V and tokens and qpos and picks and hist and step and B > 0):
            return -1
        T, tk, tp, seed = read_params(params)
        Z = flat(logits, B * (k + 1) * rs, np.float32).reshape(-1, rs)[:, :V]

        def draw(r, p):
            return int(sampling.sample_rows_np(np.array(Z[r:r + 1]), p, T, tk, tp, seed, rows=[r // (k + 1)])[0])
        return tick(draw, tokens, qpos, B, k, picks, hist, hs, hlen, pos, left, stop, step, mailbox, V)

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def speculative_emulated(chunked_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with every decode entry point up to chunked prefill and the speculative entry points."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield chunked_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return chunked_abi_emulation.counters(n)
