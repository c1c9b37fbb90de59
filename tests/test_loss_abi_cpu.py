"""include/pdn_loss.h (the masked cross entropy, prefix pdnl_) held to what tests/test_optim_abi_cpu.py holds include/pdn_optim.h
to: the library exports exactly the declared entries, they are bound beside the core header's, and every one of them is
answered by the emulator part tests/abi_emulator/_loss.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.LOSS_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_loss_entries():
    protos = _declared()
    assert len(protos) == 6 and all(n.startswith("pdnl_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.EXT_HEADER_PATHS) == 1 and _lib.EXT_HEADER_PATHS[0].endswith("pdn_optim.h")      # the pdnx_ set is as it was
    assert not set(protos) & {n for p in _lib.EXT_HEADER_PATHS for n in _lib.parse_header(p)}
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_loss.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnl_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    text = " ".join(open(_lib.LOSS_HEADER_PATHS[0]).read().replace("*", " ").split())      # (comment lines re-joined)
    assert text.count("nn/functional.py:364-381") >= len(protos) and text.count("no counterpart") >= len(protos)


def test_emulator_covers_the_loss_header(emulated_hip):
    from tests.abi_emulator import _loss, _optim
    declared = set(_declared())
    emulated = {n for n in dir(_loss.LossMixin) if n.startswith("pdnl_")}
    assert not emulated & set(_loss.NOT_EMULATED)
    assert declared - emulated == set(_loss.NOT_EMULATED)
    assert not emulated - declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _optim.extend()
    emu = _loss.extend()
    assert isinstance(emu, _loss.LossMixin) and isinstance(emu, _optim.OptimMixin)        # both parts, one on the other
    assert declared <= set(emu.protos) and _loss.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnx_grad_norm_multi_f32")
