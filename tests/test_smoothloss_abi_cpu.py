"""include/pdn_smoothloss.h (cross entropy with label_smoothing / z_loss, prefix pdnz_) held to what
tests/test_rowloss_abi_cpu.py holds include/pdn_rowloss.h to: the library exports exactly the declared entries, they are bound
beside the core header's, the set is disjoint from every other header's, and every one of them is answered by the emulator
part tests/abi_emulator/_smoothloss.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.SMOOTH_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_smooth_loss_entries():
    protos = _declared()
    assert len(protos) == 7 and all(n.startswith("pdnz_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.ROWLOSS_HEADER_PATHS) == 1 and _lib.ROWLOSS_HEADER_PATHS[0].endswith("pdn_rowloss.h")    # the pdnr_ set is as it was
    others = {n for p in _lib.EXT_HEADER_PATHS + _lib.LOSS_HEADER_PATHS + _lib.SEG_HEADER_PATHS + _lib.ROWLOSS_HEADER_PATHS
              for n in _lib.parse_header(p)}
    assert not set(protos) & others
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_smoothloss.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnz_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    text = " ".join(open(_lib.SMOOTH_HEADER_PATHS[0]).read().replace("*", " ").split())      # (comment lines re-joined)
    assert text.count("nn/functional.py:364-381") >= len(protos) and text.count("no counterpart") >= len(protos)


def test_emulator_covers_the_smooth_loss_header(emulated_hip):
    from tests.abi_emulator import _loss, _optim, _rowloss, _smoothloss
    declared = set(_declared())
    emulated = {n for n in dir(_smoothloss.SmoothLossMixin) if n.startswith("pdnz_")}
    assert not emulated & set(_smoothloss.NOT_EMULATED)
    assert declared - emulated == set(_smoothloss.NOT_EMULATED)
    assert not emulated - declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _optim.extend()
    _loss.extend()
    _rowloss.extend()
    emu = _smoothloss.extend()
    assert isinstance(emu, _smoothloss.SmoothLossMixin) and isinstance(emu, _rowloss.RowLossMixin)
    assert isinstance(emu, _loss.LossMixin) and isinstance(emu, _optim.OptimMixin)
    assert declared <= set(emu.protos) and _smoothloss.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnr_linear_ce_backward_rows_f32")


def test_emulated_counter_slot_45(emulated_hip):
    """slot 45 lies beyond the emulator's own table: the part keeps it, reports it with the others (slot 44 beside it) and
    resets it; a caller that asks for 45 counters keeps working"""
    import numpy as np
    from tests.abi_emulator import _rowloss, _smoothloss
    _rowloss.extend()
    emu = _smoothloss.extend()
    w, b, out = np.arange(12, dtype=np.float32).reshape(3, 4), np.array([1, 2, 3, 4.5], np.float32), np.zeros(4, np.float32)
    assert emu.pdnz_weight_sums_f32(w.ctypes.data, b.ctypes.data, 3, 4, out.ctypes.data, 0) == 0
    assert out.tolist() == [6.0, 22.0, 38.0, 10.5]
    assert emu.pdnz_weight_sums_f32(w.ctypes.data, None, 3, 4, out.ctypes.data, 0) == 0 and out[3] == 0.0
    buf = (ctypes.c_int64 * 46)()
    assert emu.pdn_kernel_counters(buf, 45, 0) == 0 and buf[45] == 0 and buf[44] == 0
    assert emu.pdn_kernel_counters(buf, 46, 1) == 0 and buf[45] == 2 and buf[44] == 0
    assert emu.pdn_kernel_counters(buf, 46, 0) == 0 and buf[45] == 0
