"""Sliding-window attention over grouped heads (6 query heads over 2 and over 1 key/value heads, 65536 tokens per call):
(a) `fused.attention(..., window=W)` on the windowed shared-K/V kernels of csrc/attention_gqband.hip against (b) the same
call with `attention.use_band = False` -- the path before those kernels: the band as an additive (L, L) mask on the grouped
kernels of csrc/attention_gqa.hip -- and (c) the band kernels of csrc/attention_band.hip on K / V repeated to 6 heads, with
dK / dV summed over each group (the repeat and the sum are inside the timed step: they are what that form costs).  The three
forms alternate in one process; medians of 3 rounds of STEPS steps each, forward alone and forward + backward (the backward
entry is one call: dQ and dK/dV are not timed apart here).  usage: python tools/gqband_probe.py [hd ...]
With PROBE_ONE=1: one forward + backward of each form at hd 48, L 4096, W 256, 2 KV heads, for a kernel trace."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core import fused
from pydynet_amd.core.fused.attn import _expand_heads, _reduce_heads
from pydynet_amd.core.tensor import Graph

H, TOKENS, STEPS, ROUNDS = 6, 65536, 5, 3
ONE = bool(os.environ.get("PROBE_ONE"))
rng = np.random.default_rng(0)
FORMS = ("gqband", "mask", "repeat")


def problem(HD, L, HKV):
    B, G = TOKENS // L, H // HKV
    mk = lambda heads: pdn.Tensor(rng.standard_normal((B, L, heads, HD), dtype=np.float32), dtype=np.float32,   # noqa: E731
                                  device="hip:0", requires_grad=True)
    q, k, v, w = mk(H), mk(HKV), mk(HKV), mk(H)

    def step(form, W, backward):
        """One call of `form`; returns (`_kind`, o, dk, dv) as device arrays (dk, dv None without backward)."""
        Graph.clear()
        for t in (q, k, v):
            t.zero_grad()
        if form == "repeat":
            kx, vx = (pdn.Tensor(_expand_heads(t.data, G), copy=False, device="hip:0", requires_grad=True) for t in (k, v))
            node = fused.attention(q, kx, vx, causal=True, window=W)
            if not backward:
                return node._kind, node.data, None, None
            (node * w).sum().backward()
            return node._kind, node.data, _reduce_heads(kx.grad, G), _reduce_heads(vx.grad, G)
        fused.attention.use_band = form == "gqband"
        try:
            node = fused.attention(q, k, v, causal=True, window=W)
            if backward:
                (node * w).sum().backward()
        finally:
            fused.attention.use_band = True
        return node._kind, node.data, (k.grad if backward else None), (v.grad if backward else None)

    return B, step


if ONE:
    B, step = problem(48, 4096, 2)
    for form in FORMS:
        print(form, step(form, 256, True)[0], flush=True)
    hp.synchronize()
    sys.exit(0)

for HD in [int(a) for a in sys.argv[1:]] or [48, 128]:
    for HKV in (2, 1):
        for L in (1024, 4096):
            B, step = problem(HD, L, HKV)
            for W in (128, 256, 1024):
                times, kinds, outs = {}, {}, {}
                for rnd in range(ROUNDS + 1):                     # (round 0 warms the three forms up)
                    for form in FORMS:
                        for backward in (False, True):
                            res = step(form, W, backward)
                            hp.synchronize()
                            with hp.Timer() as t:
                                for _ in range(STEPS):
                                    step(form, W, backward)
                            if rnd:
                                times.setdefault((form, backward), []).append(t.ms / STEPS * 1e3)
                        if rnd == ROUNDS:
                            kinds[form], outs[form] = res[0], [a.get() for a in res[1:]]
                diff = {f: max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(outs["gqband"], outs[f]))
                        for f in FORMS[1:]}
                med = {key: float(np.median(ts)) for key, ts in times.items()}
                tag = f"hd {HD} H {H} Hkv {HKV} L {L} B {B} W {W} "
                for form in FORMS:
                    print(f"{tag} {form:6s} ({kinds[form]}): forward {med[(form, False)]:9.1f} us   forward + backward "
                          f"{med[(form, True)]:9.1f} us", flush=True)
                print(f"{tag} gqband / mask: forward {med[('gqband', False)] / med[('mask', False)]:.3f}   forward + backward "
                      f"{med[('gqband', True)] / med[('mask', True)]:.3f}   gqband / repeat: forward "
                      f"{med[('gqband', False)] / med[('repeat', False)]:.3f}   forward + backward "
                      f"{med[('gqband', True)] / med[('repeat', True)]:.3f}   largest relative difference of o, dk, dv: to mask "
                      f"{diff['mask']:.2e}, to repeat {diff['repeat']:.2e}", flush=True)
