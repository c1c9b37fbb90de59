"""include/pdn_normgrad.h (the RMSNorm backward folded into the layer input gradient, prefix pdng_) held to what
tests/test_abi_cpu.py and tests/test_hipnp_emulated_cpu.py hold include/pdn_hip.h to: the library exports exactly the declared
entries, and every one of them is answered by the emulator part tests/abi_emulator/_normgrad.py or listed in its
NOT_EMULATED.  The emulated entry is then held to a float64 statement of itself at a row count the split kernel never sees."""
import ctypes
import subprocess

import numpy as np

from pydynet_amd import _lib


def _declared():
    protos = {}
    for path in _lib.NORMGRAD_HEADER_PATHS:
        protos.update(_lib.parse_header(path))
    return protos


def test_library_exports_exactly_the_declared_normgrad_entries():
    protos = _declared()
    assert len(protos) == 4 and all(n.startswith("pdng_") for n in protos) and not set(protos) & set(_lib.parse_header())
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in protos:
        assert hasattr(cdll, name), f"{name} declared in include/pdn_normgrad.h but not exported"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdng_")}
    assert exported == set(protos), exported ^ set(protos)
    assert set(protos) <= set(_lib.lib().fn)                  # bound next to the core header's entries
    text = open(_lib.NORMGRAD_HEADER_PATHS[0]).read()
    assert "pdn_gemm_outres_blocks_nt_f32" in text and "pdn_rmsnorm_bwd_f32" in text and "PDN_NORM_BWD_FUSE" in text


def test_emulator_covers_the_normgrad_header(emulated_hip):
    from tests.abi_emulator import _normgrad
    declared = set(_declared())
    emulated = {n for n in dir(_normgrad.NormGradMixin) if n.startswith("pdng_")}
    assert not emulated & set(_normgrad.NOT_EMULATED)
    assert declared - emulated == set(_normgrad.NOT_EMULATED)
    assert not emulated - declared
    emu = _normgrad.extend()
    assert isinstance(emu, _normgrad.NormGradMixin) and declared <= set(emu.protos) and _normgrad.extend() is emu
    assert all(_lib.provides(n) for n in emulated)


def test_emulated_entry_is_its_statement(emulated_hip):
    from tests.abi_emulator import _normgrad
    from pydynet_amd import hipnp as hp
    L = _normgrad.extend()
    rng = np.random.default_rng(3)
    M, kb, nb, D = 40, 64, 2, 288
    a = rng.standard_normal((M, kb * nb)).astype(np.float32)
    wt = (0.1 * rng.standard_normal((nb, D, kb))).astype(np.float32)
    x = rng.standard_normal((M, D)).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    ex = rng.standard_normal((M, D)).astype(np.float32)
    rms = np.sqrt((x.astype(np.float64) ** 2).mean(-1) + 1e-6).astype(np.float32)
    dy = sum(a[:, i * kb:(i + 1) * kb].astype(np.float64) @ wt[i].astype(np.float64).T for i in range(nb))
    z = x / rms[:, None].astype(np.float64)
    dz = dy * w
    ref_dx = (dz - z * (z * dz).mean(-1, keepdims=True)) / rms[:, None] + ex
    ref_dw = (dy * z).sum(0)
    ad, wd, xd, wv, exd, rd = (hp.from_numpy(v) for v in (a, wt, x, w, ex, rms))
    dx, dw = hp.empty((M, D), np.float32), hp.from_numpy(np.ones(D, np.float32))
    assert L.query("pdng_outres_blocks_nt_rmsnorm_bwd_supported", M, kb, nb) == 1
    assert L.query("pdng_outres_blocks_nt_rmsnorm_bwd_supported", M, 48, nb) == 0
    nbytes = L.query("pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes", M, kb, nb)
    ws = hp.empty((nbytes,), np.bool_)
    L.call("pdng_outres_blocks_nt_rmsnorm_bwd_f32", ad._ptr, wd._ptr, D * kb, kb, nb, xd._ptr, wv._ptr, rd._ptr, exd._ptr,
           dx._ptr, dw._ptr, 1, M, kb * nb, ws._ptr, nbytes, hp.stream())
    assert np.abs(dx.get() - ref_dx).max() <= 1e-5 * np.abs(ref_dx).max()
    assert np.abs(dw.get() - (1 + ref_dw)).max() <= 1e-5 * np.abs(ref_dw).max()
    assert L.query("pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches", 0) == 0
    try:
        L.call("pdng_outres_blocks_nt_rmsnorm_bwd_f32", ad._ptr, wd._ptr, D * kb, kb, nb, xd._ptr, wv._ptr, rd._ptr, None,
               dx._ptr, None, 0, M, kb * nb, ws._ptr, 16, hp.stream())
    except _lib.HipLibraryError as e:
        assert e.code == -3
    else:
        raise AssertionError("a short workspace was accepted")
