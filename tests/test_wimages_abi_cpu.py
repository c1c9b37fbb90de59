"""include/pdn_wimages.h (all weight plane images of a pass in one launch; prefix pdnw_) held to what tests/test_abi_cpu.py
holds include/pdn_hip.h to: the library exports exactly the declared entries and binds them next to the core header's.  The
ABI emulator answers none of them, which is what keeps the CPU tests on the per-call path (every use in the front end asks
`provides("pdnw_set_build")` first)."""
import ctypes
import subprocess

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.WIMAGES_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_wimages_entries():
    protos = _declared()
    assert len(protos) == 10 and all(n.startswith("pdnw_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert not any(n.startswith("pdnw_") for n in _lib.parse_header())          # the core header gets no new entry
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnw_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    cdll.pdnw_desc_bytes.restype = ctypes.c_int64
    assert cdll.pdnw_desc_bytes() == 64


def test_descriptors_sizes_and_refusals_need_no_gpu():
    """the constructors, pdnw_set_bytes, bind / unbind and the counts are host code"""
    L = _lib.lib()
    nb = L.query("pdnw_desc_bytes")
    recs = ctypes.create_string_buffer(nb * 3)
    base = 1 << 20                                              # (an address: nothing is dereferenced)
    L.call("pdnw_desc_qkv", ctypes.addressof(recs), base, 288 * 288, 288, 288)
    L.call("pdnw_desc_outres", ctypes.addressof(recs) + nb, base, 768, 288, 0, 0, 0)
    L.call("pdnw_desc_down_t", ctypes.addressof(recs) + 2 * nb, base, 768, 288)
    tile, piece = 2 * 32 * 288 * 2 + 256, 2 * 288 * 32 * 2

    def up(v):
        return -(-v // 256) * 256
    assert L.query("pdnw_set_bytes", recs, 3) == up(27 * tile) + up(24 * piece + 288 * 4) + up(24 * tile)
    for name, args in (("pdnw_desc_qkv", (base, 288 * 288, 288, 256)), ("pdnw_desc_gateup", (base, 100, 768, 288)),
                       ("pdnw_desc_down_t", (base + 4, 768, 288)), ("pdnw_desc_outres", (base, 8192, 288, 0, 0, 0)),
                       ("pdnw_desc_outres", (base, 864, 288, 0, 288, 288 * 288))):
        try:
            L.call(name, ctypes.addressof(recs), *args)
        except _lib.HipLibraryError as e:
            assert e.code < 0
        else:
            raise AssertionError(f"{name}{args} was accepted")
    b, h, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    L.call("pdnw_stats", ctypes.byref(b), ctypes.byref(h), ctypes.byref(p), 0)
    assert b.value >= 0 and h.value >= 0 and p.value >= 0
    L.call("pdnw_unbind")
