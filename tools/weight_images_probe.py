"""time pdnw_set_build for one layer's eight images and for six layers' forward / backward sets (benchmark shapes)"""
import ctypes
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from pydynet_amd import _lib, hipnp as hp

L = _lib.lib()
K, D, F = 288, 288, 768
rng = np.random.default_rng(0)


def layer():
    qkv = hp.from_numpy(rng.standard_normal((3, K, D), dtype=np.float32))
    wo = hp.from_numpy(rng.standard_normal((D, D), dtype=np.float32))
    gu = hp.from_numpy(rng.standard_normal((2, K, F), dtype=np.float32))
    wd = hp.from_numpy(rng.standard_normal((F, D), dtype=np.float32))
    fwd = [("pdnw_desc_qkv", (qkv._ptr, K * D, D, K)), ("pdnw_desc_outres", (wo._ptr, 288, 288, 0, 0, 0)),
           ("pdnw_desc_gateup", (gu._ptr, K * F, F, K)), ("pdnw_desc_outres", (wd._ptr, 768, 288, 0, 0, 0))]
    bwd = [("pdnw_desc_outres", (qkv._ptr, 864, 288, 1, 288, K * D)), ("pdnw_desc_outres", (wo._ptr, 288, 288, 1, 0, 0)),
           ("pdnw_desc_down_t", (wd._ptr, F, K)), ("pdnw_desc_outres", (gu._ptr, 1536, 768, 1, 768, K * F))]
    return (qkv, wo, gu, wd), fwd, bwd


def time_set(name, ctors, reps=200):
    nb = L.query("pdnw_desc_bytes")
    recs = ctypes.create_string_buffer(nb * len(ctors))
    for i, (fn, args) in enumerate(ctors):
        L.call(fn, ctypes.addressof(recs) + i * nb, *args)
    nbytes = L.query("pdnw_set_bytes", recs, len(ctors))
    arena = hp.empty((nbytes // 4,), np.float32)
    for _ in range(10):
        L.call("pdnw_set_build", recs, len(ctors), arena._ptr, hp.stream())
    hp.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(reps):
            L.call("pdnw_set_build", recs, len(ctors), arena._ptr, hp.stream())
        hp.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps)
    print(f"{name}: {len(ctors)} descriptors, {nbytes / 1e6:.1f} MB arena, {best * 1e6:.1f} us per build (back to back, best of 5 x {reps})", flush=True)


keep, F6, B6 = [], [], []
for _ in range(6):
    k, f, b = layer()
    keep.append(k); F6 += f; B6 += b
time_set("one layer, forward forms", F6[:4])
time_set("one layer, backward forms", B6[:4])
time_set("one layer, all eight", F6[:4] + B6[:4])
time_set("six layers, forward set", F6)
time_set("six layers, backward set", B6)
