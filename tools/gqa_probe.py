"""Grouped-query attention at the benchmark's attention shape (batch 64, L 256, hd 48, 6 query heads over 2 and over 1
key/value heads, causal): `fused.attention` on the shared-K/V kernels of csrc/attention_gqa.hip against the same problem on
the multi-head kernels the way it had to be computed before them -- K / V repeated on the device, the resident kernels, dK / dV
summed over the group; the copies and the reduction are part of that side.  The two routes alternate in one process; medians
of 3 rounds of 20 steps each, forward alone and forward + backward (the backward entry is one call: dQ and dK/dV are not
timed apart here).  usage: python tools/gqa_probe.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core import fused
from pydynet_amd.core.tensor import Graph

B, L, H, HD, STEPS, ROUNDS = 64, 256, 6, 48, 20, 3
rng = np.random.default_rng(0)
for Hkv in (2, 1):
    mk = lambda h: pdn.Tensor(rng.standard_normal((B, L, h, HD), dtype=np.float32), dtype=np.float32, device="hip:0",   # noqa: E731
                              requires_grad=True)
    q, k, v, w = mk(H), mk(Hkv), mk(Hkv), mk(H)

    def step(backward):
        Graph.clear()
        for t in (q, k, v):
            t.zero_grad()
        node = fused.attention(q, k, v, causal=True)
        if backward:
            (node * w).sum().backward()
        return node

    times, kinds, outs = {}, {}, {}
    for rnd in range(ROUNDS + 1):                         # (round 0 warms both routes up)
        for gqa in (True, False):
            fused.attention.use_gqa = gqa
            for backward in (False, True):
                node = step(backward)
                hp.synchronize()
                with hp.Timer() as t:
                    for _ in range(STEPS):
                        step(backward)
                if rnd:
                    times.setdefault((gqa, backward), []).append(t.ms / STEPS * 1e3)
            kinds[gqa], outs[gqa] = node._kind, (node.data.get(), k.grad.get(), v.grad.get())
    fused.attention.use_gqa = True
    diff = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(outs[True], outs[False]))
    med = {key: float(np.median(ts)) for key, ts in times.items()}
    for gqa in (True, False):
        f, fb = med[(gqa, False)], med[(gqa, True)]
        print(f"H {H} Hkv {Hkv}  {'shared K/V' if gqa else 'repeated K/V'} ({kinds[gqa]}): forward {f:8.1f} us   "
              f"forward + backward {fb:8.1f} us   backward {fb - f:8.1f} us", flush=True)
    print(f"H {H} Hkv {Hkv}  shared / repeated: forward {med[(True, False)] / med[(False, False)]:.3f}   forward + backward "
          f"{med[(True, True)] / med[(False, True)]:.3f}   largest relative difference of o, dk, dv between the routes {diff:.2e}",
          flush=True)
