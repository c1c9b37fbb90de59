"""The log-probability entry points (csrc/logprobs.hip): the rows entry and the tick form, launch counter 36.  Both follow
pydynet_amd/llm/logprobs.py.
(One part of the TEST-ONLY host emulation of the pdnhip C ABI: see tests/abi_emulator/__init__.py.)"""
import numpy as np

from pydynet_amd.llm import logprobs as lp_np
from ._base import view, flat

LOGPROBS_CHUNK = 2048                            # vocabulary tokens per workgroup of csrc/logprobs.hip


def logprobs_chunks(V):
    return -(-V // LOGPROBS_CHUNK) if V > 0 else 0


def work_bytes(R, V, n):
    a = lambda x: (x + 15) // 16 * 16            # noqa: E731
    C = logprobs_chunks(V)
    return a(4 * R) + a(8 * R) + a(4 * R * C) + a(8 * R * C) + a(8 * R * C * n) if R > 0 and V > 0 else 0


def _ok(B, V, rs, n):
    return B > 0 and V > 0 and rs >= V and 0 <= n <= lp_np.MAX_N and logprobs_chunks(V) * n <= 4096


class LogprobsMixin:
    def pdn_logprobs_chunks(self, V):
        return logprobs_chunks(V)

    def pdn_logprobs_work_bytes(self, rows, V, n):
        return work_bytes(rows, V, n)

    def pdn_logprobs_rows_f32(self, logits, rs, rows, V, n, tokens, token_lp, top_ids, top_lp, work, stream):
        if rows == 0:
            return 0
        if not (logits and tokens and token_lp and work and _ok(rows, V, rs, n) and (n == 0 or (top_ids and top_lp))):
            return -1
        z = np.array(view(logits, (rows, V), (rs, 1), np.float32))
        lp = lp_np.rows(z, np.array(flat(tokens, rows, np.int64)), n)
        flat(token_lp, rows, np.float32)[...] = lp.token
        if n:
            flat(top_ids, rows * n, np.int64)[...] = lp.top_ids.reshape(-1)
            flat(top_lp, rows * n, np.float32)[...] = lp.top_logprobs.reshape(-1)
        self._count(36)
        return 0

    def pdn_logprobs_tick_f32(self, logits, rs, B, V, n, history, hist_ring, counter, records, ring, work, stream):
        if B == 0:
            return 0
        if not (logits and history and counter and records and work and _ok(B, V, rs, n) and ring > 0
                and hist_ring >= 0):
            return -1
        step = int(flat(counter, 1, np.int32)[0]) - 1
        slot = step % hist_ring if hist_ring else step
        tok = np.array(flat(int(flat(history, 1, np.int64)[0]) + 8 * slot * B, B, np.int64))
        z = np.array(view(logits, (B, V), (rs, 1), np.float32))
        W = lp_np.record_words(n)
        rec = flat(int(flat(records, 1, np.int64)[0]) + 8 * (step % ring) * B * W, B * W, np.int64)
        rec[...] = lp_np.to_records(lp_np.rows(z, tok, n)).reshape(-1)
        self._count(36)
        return 0
