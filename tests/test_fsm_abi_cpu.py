"""include/pdn_fsm.h (token-FSM constrained decoding of a decode step, prefix pdnf_) held to what
tests/test_logitedit_abi_cpu.py holds include/pdn_logitedit.h to: the library exports exactly the declared entries, they are
bound beside the core header's, the set is disjoint from every other header's, and every one of them is answered by the
emulator part tests/abi_emulator/_fsm.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.FSM_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_fsm_entries():
    protos = _declared()
    assert len(protos) == 4 and all(n.startswith("pdnf_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.EDIT_HEADER_PATHS) == 1 and _lib.EDIT_HEADER_PATHS[0].endswith("pdn_logitedit.h")   # the pdne_ set is as it was
    others = {n for p in _lib.EXT_HEADER_PATHS + _lib.LOSS_HEADER_PATHS + _lib.SEG_HEADER_PATHS + _lib.ROWLOSS_HEADER_PATHS
              + _lib.SMOOTH_HEADER_PATHS + _lib.EDIT_HEADER_PATHS + _lib.PERSAMPLE_HEADER_PATHS for n in _lib.parse_header(p)}
    assert not set(protos) & others and not any(n.startswith("pdnf_") for n in others)
    assert not any(n.startswith("pdnf_") for n in _lib.parse_header())          # the core header gets no new entry
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_fsm.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnf_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    # the prototypes as the callers pass them: pointers, the 64-bit row stride, ints
    step = protos["pdnf_fsm_step_f32"][1]
    assert len(step) == 19 and step[1] is ctypes.c_int64 and step[15] is ctypes.c_int and step[0] is ctypes.c_void_p
    assert step[8] is ctypes.c_int and step[9] is ctypes.c_int and step[10] is ctypes.c_void_p
    assert len(protos["pdnf_fsm_rows_f32"][1]) == 14 and len(protos["pdnf_fsm_reset"][1]) == 9
    assert cdll.pdnf_fsm_chunks(32000) == 32 and cdll.pdnf_fsm_chunks(1001) == 1
    assert cdll.pdnf_fsm_chunks(1025) == 2 and cdll.pdnf_fsm_chunks(0) == 0
    text = " ".join(open(_lib.FSM_HEADER_PATHS[0]).read().replace("*", " ").split())        # (comment lines re-joined)
    assert text.count("no counterpart") >= len(protos)


def test_emulator_covers_the_fsm_header(emulated_hip):
    from tests.abi_emulator import _fsm, _logitedit, _persample
    from pydynet_amd.llm.decode_plan import _FSM_ENTRIES
    declared = set(_declared())
    emulated = {n for n in dir(_fsm.FsmMixin) if n.startswith("pdnf_")}
    assert not emulated & set(_fsm.NOT_EMULATED)
    assert declared - emulated == set(_fsm.NOT_EMULATED)
    assert not emulated - declared and set(_FSM_ENTRIES) == declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _logitedit.extend()
    _persample.extend()
    emu = _fsm.extend()
    assert isinstance(emu, _fsm.FsmMixin) and isinstance(emu, _logitedit.LogitEditMixin)
    assert isinstance(emu, _persample.PerSampleMixin)
    assert declared <= set(emu.protos) and _fsm.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdne_logit_edit_step_f32")
    assert emu.pdnf_fsm_chunks(2500) == 3


def test_emulated_counter_slot_52(emulated_hip):
    """slot 52 lies beyond the emulator's own table: the part keeps it, reports it with the others (slot 48 beside it) and
    resets it; a caller that asks for 52 counters keeps working"""
    import numpy as np
    from pydynet_amd.llm import token_fsm as F
    from tests.abi_emulator import _fsm, _logitedit
    _logitedit.extend()
    emu = _fsm.extend()
    z = np.arange(8, dtype=np.float32).reshape(2, 4)
    off, tok, nxt, dfl = F.padded(F.TokenFSM([{1: 0, 2: 0}]), 2, 4)
    states = np.array([0, -1], np.int32)
    assert emu.pdnf_fsm_rows_f32(z.ctypes.data, 4, 2, 4, off.ctypes.data, tok.ctypes.data, dfl.ctypes.data, 2, 4,
                                 states.ctypes.data, None, None, None, 0) == 0
    assert z.tolist() == [[-np.inf, 1.0, 2.0, -np.inf], [4.0, 5.0, 6.0, 7.0]]
    assert emu.pdnf_fsm_rows_f32(z.ctypes.data, 3, 2, 4, off.ctypes.data, tok.ctypes.data, dfl.ctypes.data, 2, 4,
                                 states.ctypes.data, None, None, None, 0) == -1         # (a row stride below V)
    buf = (ctypes.c_int64 * 53)()
    assert emu.pdn_kernel_counters(buf, 52, 0) == 0 and buf[52] == 0 and buf[48] == 0
    assert emu.pdn_kernel_counters(buf, 53, 1) == 0 and buf[52] == 1 and buf[48] == 0
    assert emu.pdn_kernel_counters(buf, 53, 0) == 0 and buf[52] == 0
