"""include/pdn_stopseq.h (multi-token stop sequences of a decode step, prefix pdnh_) held to what tests/test_fsm_abi_cpu.py
holds include/pdn_fsm.h to: the library exports exactly the declared entries, they are bound beside the core header's, the
set is disjoint from every other header's, and every one of them is answered by the emulator part
tests/abi_emulator/_stopseq.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.STOPSEQ_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_stopseq_entries():
    protos = _declared()
    assert len(protos) == 2 and all(n.startswith("pdnh_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.FSM_HEADER_PATHS) == 1 and _lib.FSM_HEADER_PATHS[0].endswith("pdn_fsm.h")     # the pdnf_ set is as it was
    others = {n for p in _lib.EXT_HEADER_PATHS + _lib.LOSS_HEADER_PATHS + _lib.SEG_HEADER_PATHS + _lib.ROWLOSS_HEADER_PATHS
              + _lib.SMOOTH_HEADER_PATHS + _lib.EDIT_HEADER_PATHS + _lib.PERSAMPLE_HEADER_PATHS + _lib.FSM_HEADER_PATHS
              + _lib.NORMGRAD_HEADER_PATHS + _lib.NORMPLANES_HEADER_PATHS for n in _lib.parse_header(p)}
    assert not set(protos) & others and not any(n.startswith("pdnh_") for n in others)
    assert not any(n.startswith("pdnh_") for n in _lib.parse_header())          # the core header gets no new entry
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_stopseq.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnh_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    # the prototypes as the callers pass them: pointers and ints
    step, reset = protos["pdnh_stop_step"][1], protos["pdnh_stop_reset"][1]
    assert len(step) == 14 and step[0] is ctypes.c_void_p and step[2] is ctypes.c_int
    assert [step[i] for i in (6, 7, 8)] == [ctypes.c_int] * 3 and step[12] is ctypes.c_void_p
    assert len(reset) == 10 and reset[3] is ctypes.c_int and reset[5] is ctypes.c_int and reset[8] is ctypes.c_void_p
    text = " ".join(open(_lib.STOPSEQ_HEADER_PATHS[0]).read().replace("*", " ").split())    # (comment lines re-joined)
    assert text.count("no counterpart") >= len(protos)


def test_emulator_covers_the_stopseq_header(emulated_hip):
    from tests.abi_emulator import _fsm, _logitedit, _stopseq
    from pydynet_amd.llm.decode_plan import _STOPSEQ_ENTRIES
    declared = set(_declared())
    emulated = {n for n in dir(_stopseq.StopSeqMixin) if n.startswith("pdnh_")}
    assert not emulated & set(_stopseq.NOT_EMULATED)
    assert declared - emulated == set(_stopseq.NOT_EMULATED)
    assert not emulated - declared and set(_STOPSEQ_ENTRIES) == declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _logitedit.extend()
    _fsm.extend()
    emu = _stopseq.extend()
    assert isinstance(emu, _stopseq.StopSeqMixin) and isinstance(emu, _logitedit.LogitEditMixin)
    assert isinstance(emu, _fsm.FsmMixin)
    assert declared <= set(emu.protos) and _stopseq.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnf_fsm_step_f32")


def test_emulated_counter_slot_53(emulated_hip):
    """slot 53 lies beyond the emulator's own table: the part keeps it, reports it with the others (slot 52 beside it) and
    resets it; a caller that asks for 53 counters keeps working"""
    import numpy as np
    from tests.abi_emulator import _fsm, _stopseq
    _fsm.extend()
    emu = _stopseq.extend()
    sets, start, tail = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros((3, 16), np.int32)
    rows, s_set, s_len, s_first = (np.array(a, np.int32) for a in ([2, 7, 0], [4, 4, -1], [9, 9, 3], [-1, 5, 6]))
    assert emu.pdnh_stop_reset(sets.ctypes.data, start.ctypes.data, tail.ctypes.data, 3, rows.ctypes.data, 3,
                               s_set.ctypes.data, s_len.ctypes.data, s_first.ctypes.data, 0) == 0
    assert sets.tolist() == [-1, 0, 4] and start.tolist() == [3, 0, 9]      # (row 7: outside, skipped; row 1: not listed)
    assert tail[0].tolist() == [-1, 6] + [-1] * 14 and tail[1].tolist() == [0] * 16 and tail[2].tolist() == [-1] * 16
    assert emu.pdnh_stop_reset(None, start.ctypes.data, tail.ctypes.data, 3, rows.ctypes.data, 3, s_set.ctypes.data,
                               s_len.ctypes.data, s_first.ctypes.data, 0) == -1
    buf = (ctypes.c_int64 * 54)()
    assert emu.pdn_kernel_counters(buf, 53, 0) == 0 and buf[53] == 0 and buf[52] == 0
    assert emu.pdn_kernel_counters(buf, 54, 1) == 0 and buf[53] == 1 and buf[52] == 0
    assert emu.pdn_kernel_counters(buf, 54, 0) == 0 and buf[53] == 0
