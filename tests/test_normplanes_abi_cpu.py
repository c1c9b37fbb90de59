"""include/pdn_normplanes.h (projections that do not write the block norm's output, weight gradients from (x, norm_w, rms);
prefix pdnp_) held to what tests/test_abi_cpu.py and tests/test_hipnp_emulated_cpu.py hold include/pdn_hip.h to: the library
exports exactly the declared entries, and every one of them is answered by the emulator part tests/abi_emulator/_normplanes.py
or listed in its NOT_EMULATED.  The emulated weight-gradient entry is then held to a float64 statement of itself."""
import ctypes
import subprocess

import numpy as np

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.NORMPLANES_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_normplanes_entries():
    protos = _declared()
    assert len(protos) == 8 and all(n.startswith("pdnp_") for n in protos) and not set(protos) & set(_lib.parse_header())
    assert not any(n.startswith("pdnp_") for n in _lib.parse_header())          # the core header gets no new entry
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_normplanes.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnp_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    text = open(_lib.NORMPLANES_HEADER_PATHS[0]).read()
    assert "pdn_gateup_swiglu_norm_fwd_f32" in text and "pdn_qkv_rope_norm_fwd_f32" in text and "PDN_NORM_PLANES" in text
    assert "rms[t] >= sqrt(mean_d x[t][d]^2)" in text         # the contract of the bound


def test_emulator_covers_the_normplanes_header(emulated_hip):
    from tests.abi_emulator import _normplanes
    declared = set(_declared())
    emulated = {n for n in dir(_normplanes.NormPlanesMixin) if n.startswith("pdnp_")}
    assert not emulated & set(_normplanes.NOT_EMULATED)
    assert declared - emulated == set(_normplanes.NOT_EMULATED)
    assert not emulated - declared
    emu = _normplanes.extend()
    assert isinstance(emu, _normplanes.NormPlanesMixin) and declared <= set(emu.protos) and _normplanes.extend() is emu
    assert all(_lib.provides(n) for n in emulated)


def test_emulated_weight_gradient_is_its_statement(emulated_hip):
    from tests.abi_emulator import _normplanes
    from pydynet_amd import hipnp as hp
    L = _normplanes.extend()
    rng = np.random.default_rng(5)
    K, nbc, nb, D = 96, 64, 2, 288
    x = rng.standard_normal((K, D)).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    g = rng.standard_normal((K, nb * nbc + 4)).astype(np.float32)            # rows four floats further apart than they are wide
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(-1) + 1e-6).astype(np.float32)
    dw0 = rng.standard_normal((nb, D, nbc)).astype(np.float32)
    xn = x.astype(np.float64) / rms[:, None].astype(np.float64) * w
    xd, wd, rd, gd = (hp.from_numpy(v) for v in (x, w, rms, g))
    assert L.query("pdnp_norm_dw_blocks_supported", K, nbc, nb) == 1 and L.query("pdnp_norm_dw_blocks_supported", K, 30, nb) == 0
    nbytes = L.query("pdnp_norm_dw_blocks_workspace_bytes", K, nbc, nb)
    ws = hp.empty((nbytes,), np.bool_)
    for beta in (0.0, 1.0):
        dw = hp.from_numpy(dw0)
        L.call("pdnp_norm_dw_blocks_f32", xd._ptr, wd._ptr, rd._ptr, gd._ptr, nb * nbc + 4, dw._ptr, D * nbc, beta, K, nbc, nb,
               ws._ptr, nbytes, hp.stream())
        for b in range(nb):
            ref = xn.T @ g[:, b * nbc:(b + 1) * nbc].astype(np.float64) + beta * dw0[b]
            assert np.abs(dw.get()[b] - ref).max() <= 1e-5 * np.abs(ref).max()
    assert L.query("pdnp_norm_dw_blocks_plane_launches", 0) == 0
    try:
        L.call("pdnp_norm_dw_blocks_f32", xd._ptr, wd._ptr, rd._ptr, gd._ptr, nb * nbc + 4, dw._ptr, D * nbc, 0.0, K, nbc, nb,
               ws._ptr, 16, hp.stream())
    except _lib.HipLibraryError as e:
        assert e.code == -3
    else:
        raise AssertionError("a short workspace was accepted")
