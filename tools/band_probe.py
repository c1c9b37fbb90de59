"""Sliding-window attention (6 heads, about 65k tokens per call): `fused.attention(..., window=W)` on the band kernels of
csrc/attention_band.hip against (ii) the same problem the way it had to be computed before them -- the band as an additive
(L, L) mask, resident on the device, on the streaming kernels -- and (iii) plain causal attention at the same L.  The three
forms alternate in one process; medians of 3 rounds of STEPS steps each, forward alone and forward + backward (the backward
entry is one call: dQ and dK/dV are not timed apart here).  usage: python tools/band_probe.py [hd ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core import fused
from pydynet_amd.core.fused import band
from pydynet_amd.core.tensor import Graph

H, TOKENS, STEPS, ROUNDS = 6, 65536, 5, 3
rng = np.random.default_rng(0)
for HD in [int(a) for a in sys.argv[1:]] or [48, 128]:
    for L in (1024, 4096):
        B = TOKENS // L
        mk = lambda: pdn.Tensor(rng.standard_normal((B, L, H, HD), dtype=np.float32), dtype=np.float32, device="hip:0",   # noqa: E731
                                requires_grad=True)
        q, k, v, w = mk(), mk(), mk(), mk()
        for W in (128, 256, 1024):
            mask = hp.asarray(band.band_mask(L, L, 0, W, np.float32))
            forms = {"band": dict(window=W), "mask": dict(mask=mask), "causal": {}}

            def step(form, backward):
                Graph.clear()
                for t in (q, k, v):
                    t.zero_grad()
                node = fused.attention(q, k, v, causal=True, **forms[form])
                if backward:
                    (node * w).sum().backward()
                return node

            times, kinds, outs = {}, {}, {}
            for rnd in range(ROUNDS + 1):                     # (round 0 warms the three forms up)
                for form in forms:
                    for backward in (False, True):
                        node = step(form, backward)
                        hp.synchronize()
                        with hp.Timer() as t:
                            for _ in range(STEPS):
                                step(form, backward)
                        if rnd:
                            times.setdefault((form, backward), []).append(t.ms / STEPS * 1e3)
                    if rnd == ROUNDS:
                        kinds[form], outs[form] = node._kind, (node.data.get(), k.grad.get(), v.grad.get())
            diff = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(outs["band"], outs["mask"]))
            med = {key: float(np.median(ts)) for key, ts in times.items()}
            for form in forms:
                f, fb = med[(form, False)], med[(form, True)]
                print(f"hd {HD} L {L} B {B} W {W}  {form:6s} ({kinds[form]}): forward {f:9.1f} us   forward + backward {fb:9.1f} us",
                      flush=True)
            print(f"hd {HD} L {L} B {B} W {W}  band / mask: forward {med[('band', False)] / med[('mask', False)]:.3f}   "
                  f"forward + backward {med[('band', True)] / med[('mask', True)]:.3f}   band / causal: forward "
                  f"{med[('band', False)] / med[('causal', False)]:.3f}   forward + backward "
                  f"{med[('band', True)] / med[('causal', True)]:.3f}   largest relative difference of o, dk, dv between band "
                  f"and mask {diff:.2e}", flush=True)
