"""include/pdn_segattn.h (document-masked attention, prefix pdns_) held to what tests/test_loss_abi_cpu.py holds include/pdn_loss.h
to: the library exports exactly the declared entries, they are bound beside the core header's, and every one of them is
answered by the emulator part tests/abi_emulator/_segattn.py or listed in its NOT_EMULATED."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.SEG_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_segment_entries():
    protos = _declared()
    assert set(protos) == {"pdns_attention_supported", "pdns_segment_bounds_i32", "pdns_attention_fwd_f32", "pdns_attention_bwd_f32"}
    assert not set(protos) & set(_lib.parse_header())
    # the other sets are as they were
    assert len(_lib.EXT_HEADER_PATHS) == 1 and _lib.EXT_HEADER_PATHS[0].endswith("pdn_optim.h")
    assert len(_lib.LOSS_HEADER_PATHS) == 1 and _lib.LOSS_HEADER_PATHS[0].endswith("pdn_loss.h")
    for paths in (_lib.EXT_HEADER_PATHS, _lib.LOSS_HEADER_PATHS):
        assert not set(protos) & {n for p in paths for n in _lib.parse_header(p)}
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_segattn.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdns_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    # argument counts of the two attention entries: pdn_attention_fwd_f32 less `causal` plus the bounds, and the
    # backward with `prerotated` and both bounds
    core = _lib.parse_header()
    assert len(protos["pdns_attention_fwd_f32"][1]) == len(core["pdn_attention_fwd_f32"][1])
    assert len(protos["pdns_attention_bwd_f32"][1]) == len(core["pdn_attention_bwd_f32"][1]) + 2
    text = " ".join(open(_lib.SEG_HEADER_PATHS[0]).read().replace("*", " ").split())       # (comment lines re-joined)
    assert text.count("no counterpart") >= len(protos)


def test_emulator_covers_the_segment_header(emulated_hip):
    from tests.abi_emulator import _loss, _optim, _segattn
    declared = set(_declared())
    emulated = {n for n in dir(_segattn.SegAttnMixin) if n.startswith("pdns_")}
    assert not emulated & set(_segattn.NOT_EMULATED)
    assert declared - emulated == set(_segattn.NOT_EMULATED)
    assert not emulated - declared
    assert not any(_lib.provides(n) for n in declared)        # the core registry does not know them
    _optim.extend()
    _loss.extend()
    emu = _segattn.extend()
    assert isinstance(emu, _segattn.SegAttnMixin) and isinstance(emu, _loss.LossMixin) and isinstance(emu, _optim.OptimMixin)
    assert declared <= set(emu.protos) and _segattn.extend() is emu
    assert all(_lib.provides(n) for n in emulated) and _lib.provides("pdnl_linear_ce_finish_f32")
    # launch counter slot 43 lies beyond the emulator's own table: this part keeps it, and reports and resets it with the rest
    buf = (ctypes.c_int64 * 44)()
    emu._count(43)
    emu._count(9)
    emu.call("pdn_kernel_counters", buf, 44, 1)
    assert buf[43] == 1 and buf[9] == 1
    emu.call("pdn_kernel_counters", buf, 44, 0)
    assert buf[43] == 0 and buf[9] == 0
