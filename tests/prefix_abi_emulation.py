"""TEST-ONLY NumPy statement of the prefix-caching entry point of include/pdn_hip.h (csrc/prefix.hip: the row-to-row copy
of `Llama.serve(prefix_cache=...)`), attached to the emulated library of tests/abi_emulator by the `prefix_emulated` fixture
below, with launch counter 38 (37 is the split-fp16 lm_head, which the emulated library does not run; 36 the
log-probabilities of tests/logprobs_abi_emulation.py).  `copy_prefix_np` is also the reference of the GPU test."""
import ctypes

import numpy as np
import pytest

from tests import logprobs_abi_emulation
from tests.abi_emulator import flat, view
from tests.logprobs_abi_emulation import logprobs_emulated  # noqa: F401  (fixture)

SLOTS = 39
MAX_COPIES = 256


def copy_prefix_np(caches, dst, src, lens):
    """pdn_kv_copy_prefix_rows_f32 on arrays: each cache (n_rows, max_len, D), written in place.  Snapshot, then copy:
    every source is read as it was before the call."""
    for c in caches:
        n_rows, max_len = c.shape[:2]
        before = np.array(c)
        for d, s, n in zip(np.asarray(dst).tolist(), np.asarray(src).tolist(), np.asarray(lens).tolist()):
            if d == s or n <= 0 or not (0 <= d < n_rows and 0 <= s < n_rows):
                continue
            n = min(n, max_len)
            c[d, :n] = before[s, :n]


def attach(monkeypatch, emu):
    count = [0]
    base_counters = emu.pdn_kernel_counters

    def pdn_kernel_counters(out, n, reset):
        base_counters(out, n, reset)
        if out and int(n) > 38:
            ctypes.cast(out, ctypes.POINTER(ctypes.c_int64))[38] = count[0]
        if reset:
            count[0] = 0
        return 0

    def pdn_kv_copy_prefix_rows_f32(caches, n_tensors, bs, n_rows, max_len, D, dst, src, lens, n_copies, stream):
        if n_tensors == 0 or n_copies == 0:
            return 0
        if not (caches and dst and src and lens and n_tensors > 0 and n_rows > 0 and 0 < n_copies <= MAX_COPIES
                and max_len > 0 and D > 0 and bs >= max_len * D):
            return -1
        ptrs = np.array(flat(caches, n_tensors, np.int64))
        copy_prefix_np([view(int(p), (n_rows, max_len, D), (bs, D, 1), np.float32) for p in ptrs],
                       *(np.array(flat(a, n_copies, np.int32)) for a in (dst, src, lens)))
        count[0] += 1
        return 0

    for name, f in list(locals().items()):
        if name.startswith("pdn_"):
            monkeypatch.setattr(emu, name, f, raising=False)
    return emu


@pytest.fixture()
def prefix_emulated(logprobs_emulated, monkeypatch):  # noqa: F811
    """The emulated C ABI with every decode entry point up to the log-probabilities and the prefix copy."""
    from pydynet_amd import _lib
    attach(monkeypatch, _lib._LIB)
    yield logprobs_emulated


def counters(n=SLOTS):
    """Launch counters 0 .. n-1 since the last call (reset after reading)."""
    return logprobs_abi_emulation.counters(n)
