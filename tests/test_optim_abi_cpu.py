"""include/pdn_optim.h (the extension entries, prefix pdnx_) held to what tests/test_abi_cpu.py and tests/test_hipnp_emulated_cpu.py
hold include/pdn_hip.h to: the library exports exactly the declared entries, and every one of them is answered by the emulator
part tests/abi_emulator/_optim.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.EXT_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_extension_entries():
    protos = _declared()
    assert len(protos) == 4 and all(n.startswith("pdnx_") for n in protos) and not set(protos) & set(_lib.parse_header())
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_optim.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnx_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    text = open(_lib.EXT_HEADER_PATHS[0]).read()
    assert "optim/optimizer.py:185-196" in text and "no counterpart" in text


def test_emulator_covers_the_extension_header(emulated_hip):
    from tests.abi_emulator import _optim
    declared = set(_declared())
    emulated = {n for n in dir(_optim.OptimMixin) if n.startswith("pdnx_")}
    assert not emulated & set(_optim.NOT_EMULATED)
    assert declared - emulated == set(_optim.NOT_EMULATED)
    assert not emulated - declared
    emu = _optim.extend()
    assert isinstance(emu, _optim.OptimMixin) and declared <= set(emu.protos) and _optim.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and not _lib.provides(_optim.NOT_EMULATED[0])
