"""include/pdn_rowloss.h (cross entropy with reduction='none', prefix pdnr_) held to what tests/test_loss_abi_cpu.py holds
include/pdn_loss.h to: the library exports exactly the declared entries, they are bound beside the core header's, and every one
of them is answered by the emulator part tests/abi_emulator/_rowloss.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.ROWLOSS_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_row_loss_entries():
    protos = _declared()
    assert len(protos) == 7 and all(n.startswith("pdnr_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.LOSS_HEADER_PATHS) == 1 and _lib.LOSS_HEADER_PATHS[0].endswith("pdn_loss.h")      # the pdnl_ set is as it was
    others = {n for p in _lib.EXT_HEADER_PATHS + _lib.LOSS_HEADER_PATHS + _lib.SEG_HEADER_PATHS for n in _lib.parse_header(p)}
    assert not set(protos) & others
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_rowloss.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnr_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    text = " ".join(open(_lib.ROWLOSS_HEADER_PATHS[0]).read().replace("*", " ").split())      # (comment lines re-joined)
    assert text.count("nn/functional.py:364-381") >= len(protos) and text.count("no counterpart") >= len(protos)


def test_emulator_covers_the_row_loss_header(emulated_hip):
    from tests.abi_emulator import _loss, _optim, _rowloss
    declared = set(_declared())
    emulated = {n for n in dir(_rowloss.RowLossMixin) if n.startswith("pdnr_")}
    assert not emulated & set(_rowloss.NOT_EMULATED)
    assert declared - emulated == set(_rowloss.NOT_EMULATED)
    assert not emulated - declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _optim.extend()
    _loss.extend()
    emu = _rowloss.extend()
    assert isinstance(emu, _rowloss.RowLossMixin) and isinstance(emu, _loss.LossMixin) and isinstance(emu, _optim.OptimMixin)
    assert declared <= set(emu.protos) and _rowloss.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnl_linear_ce_finish_f32")


def test_emulated_counter_slot_44(emulated_hip):
    """slot 44 lies beyond the emulator's own table: the part keeps it, reports it with the others and resets it"""
    import numpy as np
    from tests.abi_emulator import _rowloss
    emu = _rowloss.extend()
    u, safe, out = np.array([0.5, -3.0, 9.0], np.float32), np.array([1, 2, 4], np.int64), np.zeros(2, np.float32)
    assert emu.pdnr_abs_max_rows_f32(u.ctypes.data, safe.ctypes.data, 4, 3, out.ctypes.data, 0) == 0
    assert out[0] == 3.0 and out[1] == np.float32(1) / np.float32(3)       # (row 2 is an ignored row: its 9 does not count)
    buf = (ctypes.c_int64 * 45)()
    assert emu.pdn_kernel_counters(buf, 45, 1) == 0 and buf[44] == 1
    assert emu.pdn_kernel_counters(buf, 45, 0) == 0 and buf[44] == 0
