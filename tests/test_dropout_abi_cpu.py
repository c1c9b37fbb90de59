"""include/pdn_dropout.h (prefix pdnd_) held to what tests/test_stopseq_abi_cpu.py holds include/pdn_stopseq.h to: header,
the library's pdnd_* exports and the emulator part tests/abi_emulator/_dropout.py are equal."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    return _lib.parse_header(_lib.DROPOUT_HEADER_PATHS[0])


def test_library_exports_exactly_the_declared_dropout_entries():
    protos = _declared()
    assert len(protos) == 5 and all(n.startswith("pdnd_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert not any(n.startswith("pdnd_") for n in _lib.parse_header())          # the core header gets no new entry
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnd_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    fwd = protos["pdnd_dropout_fwd_f32"][1]                   # p a double, n 64-bit
    assert fwd == protos["pdnd_dropout_bwd_f32"][1] and fwd[2] is ctypes.c_int64 and fwd[3] is ctypes.c_double


def test_emulator_covers_the_dropout_header(emulated_hip):
    from tests.abi_emulator import _dropout, _stopseq
    declared = set(_declared())
    emulated = {n for n in dir(_dropout.DropoutMixin) if n.startswith("pdnd_")}
    assert not emulated & set(_dropout.NOT_EMULATED) and declared - emulated == set(_dropout.NOT_EMULATED)
    assert not emulated - declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _stopseq.extend()
    emu = _dropout.extend()
    assert isinstance(emu, _dropout.DropoutMixin) and isinstance(emu, _stopseq.StopSeqMixin)
    assert declared <= set(emu.protos) and _dropout.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnh_stop_step")
