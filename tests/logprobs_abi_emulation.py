"""TEST-ONLY NumPy statements of the log-probability entry points of include/pdn_hip.h (csrc/logprobs.hip: the rows entry
and the tick form), attached to the emulated library of tests/abi_emulator by the `logprobs_emulated` fixture below, with
launch counter 36 next to the penalty slot 35 (tests/penalty_abi_emulation.py).  Both follow
pydynet_amd/llm/logprobs.py."""
import ctypes

import numpy as np
import pytest

from pydynet_amd.llm import logprobs as lp_np
from tests import penalty_abi_emulation
from tests.abi_emulator import flat, view
from tests.penalty_abi_emulation import penalty_emulated  # noqa: F401  (fixture)

SLOTS = 37
CHUNK = 2048                                     # vocabulary tokens per workgroup of csrc/logprobs.hip


def chunks(V):
    return -(-V // CHUNK) if V > 0 else 0


def work_bytes(R, V, n):
    a = lambda x: (x + 15) // 16 * 16            # noqa: E731
    C = chunks(V)
    return a(4 * R) + a(8 * R) + a(4 * R * C) + a(8 * R * C) + a(8 * R * C * n) if R > 0 and V > 0 else 0


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 36:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[36] = count[0]
        if reset:
            count[0] = 0
        return 0

    def pdn_logprobs_chunks(V):
        return chunks(V)

    def pdn_logprobs_work_bytes(rows, V, n):
        return work_bytes(rows, V, n)

    def ok(B, V, rs, n):
        return B > 0 and V > 0 and rs >= V and 0 <= n <= lp_np.MAX_N and chunks(V) * n <= 4096

    def pdn_logprobs_rows_f32(logits, rs, rows, V, n, tokens, token_lp, top_ids, top_lp, work, stream):
        if rows == 0:
            return 0
        if not (logits and tokens and token_lp and work and ok(rows, V, rs, n) and (n == 0 or (top_ids and top_lp))):
            return -1
        z = np.array(view(logits, (rows, V), (rs, 1), np.float32))
        lp = lp_np.rows(z, np.array(flat(tokens, rows, np.int64)), n)
        flat(token_lp, rows, np.float32)[...] = lp.token
        if n:
            flat(top_ids, rows * n, np.int64)[...] = lp.top_ids.reshape(-1)
            flat(top_lp, rows * n, np.float32)[...] = lp.top_logprobs.reshape(-1)
        count[0] += 1
        return 0

    def pdn_logprobs_tick_f32(logits, rs, B, V, n, history, hist_ring, counter, records, ring, work, stream):
        if B == 0:
            return 0
        if not (logits and history and counter and records and work and ok(B, V, rs, n) and ring > 0
                and hist_ring >= 0):
            return -1
        step = int(flat(counter, 1, np.int32)[0]) - 1
        slot = step % hist_ring if hist_ring else step
        tok = np.array(flat(int(flat(history, 1, np.int64)[0]) + 8 * slot * B, B, np.int64))
        z = np.array(view(logits, (B, V), (rs, 1), np.float32))
        W = lp_np.record_words(n)
        rec = flat(int(flat(records, 1, np.int64)[0]) + 8 * (step % ring) * B * W, B * W, np.int64)
        rec[...] = lp_np.to_records(lp_np.rows(z, tok, n)).reshape(-1)
        count[0] += 1
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def logprobs_emulated(penalty_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with every decode entry point up to the penalties and the log-probability entry points."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield penalty_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return penalty_abi_emulation.counters(n)
