"""include/pdn_persample.h (sampling parameters per row, prefix pdnq_) held to what tests/test_logitedit_abi_cpu.py holds
include/pdn_logitedit.h to: the library exports exactly the declared entries, they are bound beside the core header's, the
set is disjoint from every other header's, and every one of them is answered by the emulator part
tests/abi_emulator/_persample.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

import numpy as np

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.PERSAMPLE_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_per_row_sampling_entries():
    protos = _declared()
    assert len(protos) == 6 and all(n.startswith("pdnq_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert len(_lib.EDIT_HEADER_PATHS) == 1 and _lib.EDIT_HEADER_PATHS[0].endswith("pdn_logitedit.h")   # the pdne_ set is as it was
    others = {n for p in _lib.EXT_HEADER_PATHS + _lib.LOSS_HEADER_PATHS + _lib.SEG_HEADER_PATHS + _lib.ROWLOSS_HEADER_PATHS
              + _lib.SMOOTH_HEADER_PATHS + _lib.EDIT_HEADER_PATHS for n in _lib.parse_header(p)}
    assert not set(protos) & others and not any(n.startswith("pdnq_") for n in others)
    assert not any(n.startswith("pdnq_") for n in _lib.parse_header())          # the core header gets no new entry
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_persample.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnq_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    # every entry takes the arguments of the shared-parameter entry it is named after, in the same order
    core = _lib.parse_header()
    for name, (ret, args) in protos.items():
        if name == "pdnq_sample_rows_f32":
            assert len(args) == 9 and args[1] is ctypes.c_int64 and args[5] is ctypes.c_void_p and args[6] is ctypes.c_void_p
        else:
            assert (ret, args) == core["pdn_" + name[len("pdnq_"):]], name
    text = " ".join(open(_lib.PERSAMPLE_HEADER_PATHS[0]).read().replace("*", " ").split())  # (comment lines re-joined)
    assert text.count("no counterpart") >= 4 and "min_p" in text and "slot 49" in text


def test_emulator_covers_the_per_row_sampling_header(emulated_hip):
    from tests.abi_emulator import _logitedit, _persample
    from pydynet_amd.llm.decode_plan import _PERSAMPLE_ENTRIES
    declared = set(_declared())
    emulated = {n for n in dir(_persample.PerSampleMixin) if n.startswith("pdnq_")}
    assert not emulated & set(_persample.NOT_EMULATED)
    assert declared - emulated == set(_persample.NOT_EMULATED)
    assert not emulated - declared and set(_PERSAMPLE_ENTRIES) == declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _logitedit.extend()
    emu = _persample.extend()
    assert isinstance(emu, _persample.PerSampleMixin) and isinstance(emu, _logitedit.LogitEditMixin)
    assert declared <= set(emu.protos) and _persample.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdne_logit_edit_step_f32")


def test_emulated_counter_slot_49_and_the_standalone_entry(emulated_hip):
    """slot 49 lies beyond the emulator's own table: the part keeps it, reports it beside slot 48 and resets it; the
    standalone entry draws each live row under its own block and leaves a row at a position < 0 alone"""
    from pydynet_amd.llm import sampling
    from tests.abi_emulator import _logitedit, _persample
    _logitedit.extend()
    emu = _persample.extend()
    z = np.random.default_rng(0).standard_normal((3, 40)).astype(np.float32) * 3
    tab = sampling.Table([0.0, 1.0, 0.7], [0, 0, 4], [1.0, 0.8, 1.0], [5, 6, 7], [0.0, 0.0, 0.2])
    prm, pos, req = tab.blocks([0, 1, 2]), np.array([4, -1, 9], np.int32), np.array([8, 2, 5], np.int32)
    out = np.full(3, -7, np.int64)
    assert emu.pdnq_sample_rows_f32(z.ctypes.data, 40, 3, 40, prm.ctypes.data, pos.ctypes.data, req.ctypes.data,
                                    out.ctypes.data, 0) == 0
    want2 = sampling.sample_rows_np(z[2:3], 9, np.float32(0.7), 4, 1.0, 7, rows=[5], min_p=np.float32(0.2))[0]
    assert out.tolist() == [int(z[0].argmax()), -7, int(want2)]
    assert emu.pdnq_sample_rows_f32(z.ctypes.data, 39, 3, 40, prm.ctypes.data, pos.ctypes.data, None, out.ctypes.data,
                                    0) == -1                                       # (a row stride below V)
    assert _persample.read_block(prm[2]) == (float(np.float32(0.7)), 4, 1.0, 7, float(np.float32(0.2)))
    buf = (ctypes.c_int64 * 50)()
    assert emu.pdn_kernel_counters(buf, 49, 0) == 0 and buf[49] == 0
    assert emu.pdn_kernel_counters(buf, 50, 1) == 0 and buf[49] == 1 and buf[48] == 0 and buf[28] == 1
    assert emu.pdn_kernel_counters(buf, 50, 0) == 0 and buf[49] == 0
