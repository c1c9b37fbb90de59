"""include/pdn_logitedit.h (the per-request logit edits of a decode step, prefix pdne_) held to what
tests/test_smoothloss_abi_cpu.py holds include/pdn_smoothloss.h to: the library exports exactly the declared entries, they are
bound beside the core header's, the set is disjoint from every other header's, and every one of them is answered by the
emulator part tests/abi_emulator/_logitedit.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.EDIT_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_logit_edit_entries():
    protos = _declared()
    assert len(protos) == 4 and all(n.startswith("pdne_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.SMOOTH_HEADER_PATHS) == 1 and _lib.SMOOTH_HEADER_PATHS[0].endswith("pdn_smoothloss.h")   # the pdnz_ set is as it was
    others = {n for p in _lib.EXT_HEADER_PATHS + _lib.LOSS_HEADER_PATHS + _lib.SEG_HEADER_PATHS + _lib.ROWLOSS_HEADER_PATHS
              + _lib.SMOOTH_HEADER_PATHS for n in _lib.parse_header(p)}
    assert not set(protos) & others and not any(n.startswith("pdne_") for n in others)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_logitedit.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdne_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    # the prototypes as the callers pass them: pointers, the 64-bit row stride, ints
    step = protos["pdne_logit_edit_step_f32"][1]
    assert len(step) == 17 and step[1] is ctypes.c_int64 and step[12] is ctypes.c_int and step[0] is ctypes.c_void_p
    assert len(protos["pdne_logit_edit_rows_f32"][1]) == 16 and len(protos["pdne_logit_edit_reset"][1]) == 17
    assert cdll.pdne_logit_edit_chunks(32000) == 32 and cdll.pdne_logit_edit_chunks(1001) == 1
    assert cdll.pdne_logit_edit_chunks(1025) == 2 and cdll.pdne_logit_edit_chunks(0) == 0
    text = " ".join(open(_lib.EDIT_HEADER_PATHS[0]).read().replace("*", " ").split())       # (comment lines re-joined)
    assert text.count("no counterpart") >= len(protos) and "#define PDNE_MAX_BIAS 1024" in text


def test_emulator_covers_the_logit_edit_header(emulated_hip):
    from tests.abi_emulator import _logitedit, _rowloss, _smoothloss
    from pydynet_amd.llm import logit_edits
    from pydynet_amd.llm.decode_plan import _EDIT_ENTRIES
    declared = set(_declared())
    emulated = {n for n in dir(_logitedit.LogitEditMixin) if n.startswith("pdne_")}
    assert not emulated & set(_logitedit.NOT_EMULATED)
    assert declared - emulated == set(_logitedit.NOT_EMULATED)
    assert not emulated - declared and set(_EDIT_ENTRIES) == declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _rowloss.extend()
    _smoothloss.extend()
    emu = _logitedit.extend()
    assert isinstance(emu, _logitedit.LogitEditMixin) and isinstance(emu, _smoothloss.SmoothLossMixin)
    assert isinstance(emu, _rowloss.RowLossMixin)
    assert declared <= set(emu.protos) and _logitedit.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnz_weight_sums_f32")
    assert emu.pdne_logit_edit_chunks(2500) == 3 and logit_edits.MAX_BIAS == 1024


def test_emulated_counter_slot_48(emulated_hip):
    """slot 48 lies beyond the emulator's own table: the part keeps it, reports it with the others (slot 45 beside it) and
    resets it; a caller that asks for 48 counters keeps working"""
    import numpy as np
    from pydynet_amd.llm import logit_edits
    from tests.abi_emulator import _logitedit, _smoothloss
    _smoothloss.extend()
    emu = _logitedit.extend()
    z = np.arange(8, dtype=np.float32).reshape(2, 4)
    prm = logit_edits.params_bytes(0)
    bits, on = logit_edits.allow_bits([[1, 2], None], 4)
    assert emu.pdne_logit_edit_rows_f32(z.ctypes.data, 4, 2, 4, prm.ctypes.data, bits.ctypes.data, on.ctypes.data, None, None,
                                        None, None, None, None, None, None, 0) == 0
    assert z.tolist() == [[-np.inf, 1.0, 2.0, -np.inf], [4.0, 5.0, 6.0, 7.0]]
    assert emu.pdne_logit_edit_rows_f32(z.ctypes.data, 3, 2, 4, prm.ctypes.data, None, None, None, None, None, None, None,
                                        None, None, None, 0) == -1                    # (a row stride below V)
    buf = (ctypes.c_int64 * 49)()
    assert emu.pdn_kernel_counters(buf, 48, 0) == 0 and buf[48] == 0 and buf[45] == 0
    assert emu.pdn_kernel_counters(buf, 49, 1) == 0 and buf[48] == 1 and buf[45] == 0
    assert emu.pdn_kernel_counters(buf, 49, 0) == 0 and buf[48] == 0
