"""What the device-drawn dropout costs (csrc/dropout.hip, core/fused/dropout.py).
  kernels   pdnd_dropout_fwd_f32 / _bwd_f32 / _add_fwd_f32 over 131072 x 288 floats against the library's own elementwise scale
            (x * c, the same 8 bytes per element; dropout_add moves 12) and against the host-drawn nn.Dropout over the same
            array, upload included; the same kernels at the Llama step's array (64 x 256 x 288) for the split below.  Device
            events around `reps` launches; under `rocprofv3 --kernel-trace --stats -- python tools/dropout_probe.py kernels`
            the trace gives the per-launch kernel times, which `stats` turns into the table.
  llama     the six-layer Llama (V 32000, D 288, 6 heads, F 768) at seq 256, batch 64: `finetune_step` with dropout=0.0 and
            with dropout=0.1, two models alternating in one process, medians of `rounds` rounds of `steps` steps; the difference
            split into the dropout launches (1 forward, 12 dropout_add, 13 backward, 13 claims, from the figures of `kernels`
            measured in the same process) and the rest: the two residual epilogues per layer that the dropout path gives up.
  folds     a 2-layer Llama (V 2048, D 288, seq 256) with dropout=0.1 at batch x 256 rows: loss and every parameter gradient of
            one forward / backward with the folds around the residual stream on (the deferred rms_norm, its backward in the
            input-gradient drain, the never-written norm planes, the weight images) against all of them off, both from
            generator state (0, 0): the worst relative difference, and the plane launches that show the fold ran.
usage: python tools/dropout_probe.py kernels [reps=20]
       python tools/dropout_probe.py folds [batch=256]
       python tools/dropout_probe.py llama [rounds=3] [steps=10] [batch=64]
       python tools/dropout_probe.py stats KERNEL_STATS.csv"""
import json
import os
import sys

mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
ROWS, COLS = 131072, 288
if mode == "stats":
    import csv
    for r in csv.DictReader(open(sys.argv[2])):
        name = r["Name"]
        avg = float(r["AverageNs"])
        if int(r["Calls"]) >= 10:                            # (the timed windows; one-off set-up launches are left out)
            print(f"{name[:70]:70s} calls {r['Calls']:>5s}  avg {avg / 1e3:9.2f} us  min {float(r['MinNs']) / 1e3:9.2f} us  "
                  f"max {float(r['MaxNs']) / 1e3:9.2f} us")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp, nn, _lib
from pydynet_amd.core.tensor import Graph

hp.set_device(0)
L = _lib.lib()


def timed(fn, reps, rounds=5):
    """Median and span over `rounds` of the device time of one call, `reps` calls between two events."""
    fn()
    hp.synchronize()
    ms = []
    for _ in range(rounds):
        a = hp.Event().record()
        for _ in range(reps):
            fn()
        b = hp.Event().record()
        ms.append(a.elapsed_ms(b) / reps)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def kernel_times(n, reps):
    """us per launch of the three dropout entries, the claim and the scale kernel over n floats."""
    rng = np.random.default_rng(0)
    x = hp.from_numpy(rng.standard_normal(n).astype(np.float32))
    r = hp.from_numpy(rng.standard_normal(n).astype(np.float32))
    y = hp.empty((n,), np.float32)
    gen = pdn.Generator(1, "hip:0")
    slot = gen.claim(n)
    st = hp.stream()
    calls = {
        "scale x * c": lambda: x * 1.25,
        "pdnd_dropout_fwd_f32": lambda: L.call("pdnd_dropout_fwd_f32", x._ptr, y._ptr, n, 0.1, slot._ptr, st),
        "pdnd_dropout_bwd_f32": lambda: L.call("pdnd_dropout_bwd_f32", x._ptr, y._ptr, n, 0.1, slot._ptr, st),
        "pdnd_dropout_add_fwd_f32": lambda: L.call("pdnd_dropout_add_fwd_f32", x._ptr, r._ptr, y._ptr, n, 0.1, slot._ptr, st),
        "pdnd_rng_claim": lambda: L.call("pdnd_rng_claim", gen._state._ptr, slot._ptr, n, st),
    }
    out = {}
    for _ in range(2):                                       # twice, alternating: the second pass is reported
        for name, fn in calls.items():
            out[name] = timed(fn, reps)
    return {k: tuple(1e3 * v for v in t) for k, t in out.items()}


def report(n, times):
    base = times["scale x * c"][0]
    for name, (med, lo, hi) in times.items():
        nbytes = {"pdnd_dropout_add_fwd_f32": 12, "pdnd_rng_claim": 0}.get(name, 8) * n
        rate = f"{nbytes / med / 1e6:7.2f} TB/s" if nbytes else ""
        print(f"  {name:28s} {med:9.2f} us  (span {lo:.2f} .. {hi:.2f})  {med / base:6.3f} x scale  {rate}")


if mode == "folds":
    from pydynet_amd.core import fused
    from pydynet_amd.llm.llama import Llama
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    V, D, SEQ = 2048, 288, 256
    rng = np.random.default_rng(1)
    ids, tgt = rng.integers(0, V, (batch, SEQ)), rng.integers(0, V, batch * SEQ)

    def run(on):
        fused.rms_norm.fold = fused.rms_norm.fuse_bwd = fused.ffn_swiglu.norm_planes = fused.qkv_attention.norm_planes = on
        os.environ["PDN_WIMAGES"] = "1" if on else "0"
        Graph.clear()
        np.random.seed(0)
        m = Llama(V, D, 6, 768, SEQ, 1, 2, np.float32, dropout=0.1)
        m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
        m.to("hip:0")
        for p in m.parameters():
            p.zero_grad()
        L.query("pdnp_norm_dw_blocks_plane_launches", 1)
        loss = m.loss(ids, tgt)
        loss.backward()
        return (float(loss.item()), {n: p.grad.get() for n, p in m.named_parameters()},
                L.query("pdnp_norm_dw_blocks_plane_launches", 1), m.generator.get_state())
    a, b = run(True), run(False)
    errs = {n: float(np.abs(a[1][n] - b[1][n]).max()) / float(np.abs(b[1][n]).max()) for n in a[1]}
    worst = max(errs, key=errs.get)
    print(f"{batch * SEQ} rows: loss folds on {a[0]:.6f} / off {b[0]:.6f}, generator after {a[3]} / {b[3]}, plane launches {a[2]} / {b[2]}")
    print(f"  {len(errs)} parameter gradients, worst relative difference {errs[worst]:.3e} ({worst})")
    assert a[3] == b[3] and errs[worst] <= 1e-4 and abs(a[0] - b[0]) <= 1e-4 * abs(b[0])       # the project's fp32 parity bound
    sys.exit(0)

if mode == "kernels":
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    n = ROWS * COLS
    print(f"{ROWS} x {COLS} floats ({4 * n / 1e6:.1f} MB per array), {reps} launches per window, medians of 5 windows")
    big = kernel_times(n, reps)
    report(n, big)
    xh = np.random.default_rng(0).standard_normal((ROWS, COLS)).astype(np.float32)
    xt = pdn.Tensor(xh, device="hip:0")
    host_layer, dev_layer = nn.Dropout(0.1), nn.Dropout(0.1, generator=pdn.Generator(1, "hip:0"))

    def host_drawn():
        host_layer(xt)
        hp.synchronize()
    import time
    host_drawn()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_drawn()
        t.append(1e3 * (time.perf_counter() - t0))
    med, lo, hi = timed(lambda: dev_layer(xt), reps)
    print(f"  nn.Dropout(0.1), host draw + upload + three launches: {np.median(t):9.2f} ms per call (host clock, {min(t):.2f} .. {max(t):.2f})")
    print(f"  nn.Dropout(0.1, generator): claim + forward:           {med:9.4f} ms per call ({lo:.4f} .. {hi:.4f})")
    print(json.dumps({"n": n, "us": {k: v[0] for k, v in big.items()}, "host_drawn_ms": float(np.median(t)), "device_drawn_ms": med}))
    sys.exit(0)

from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam

rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
batch = int(sys.argv[4]) if len(sys.argv) > 4 else 64
V, D, H, F_, SEQ, LAYERS = 32000, 288, 6, 768, 256, 6
rng = np.random.default_rng(1)
ids = pdn.Tensor(rng.integers(0, V, (batch, SEQ)), dtype=np.int64, device="hip:0")
tgt = pdn.Tensor(rng.integers(0, V, (batch * SEQ,)), dtype=np.int64, device="hip:0")
Graph.clear()
runs = {}
for p in (0.0, 0.1):
    np.random.seed(0)
    m = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32, dropout=p)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    m.to("hip:0")
    runs[p] = (m, Adam(m.parameters(), lr=1e-4))
for m, opt in runs.values():
    for _ in range(2):
        m.finetune_step(ids, tgt, opt)
ms, loss = {p: [] for p in runs}, {}
for _ in range(rounds):
    for p, (m, opt) in runs.items():
        hp.synchronize()
        a = hp.Event().record()
        for _ in range(steps):
            loss[p] = m.finetune_step(ids, tgt, opt)
        b = hp.Event().record()
        ms[p].append(a.elapsed_ms(b) / steps)
med = {p: float(np.median(v)) for p, v in ms.items()}
for p in runs:
    print(f"dropout={p}: {med[p]:8.3f} ms/step  rounds {[round(x, 3) for x in ms[p]]}  loss {loss[p]:.4f}")
n = batch * SEQ * D
k = kernel_times(n, 50)
print(f"the dropout launches at {batch} x {SEQ} x {D} floats:")
report(n, k)
launches = (k["pdnd_dropout_fwd_f32"][0] + 2 * LAYERS * k["pdnd_dropout_add_fwd_f32"][0]
            + (2 * LAYERS + 1) * (k["pdnd_dropout_bwd_f32"][0] + k["pdnd_rng_claim"][0])) / 1e3
diff = med[0.1] - med[0.0]
print(f"difference {diff:.3f} ms/step = {100 * diff / med[0.0]:.2f} %: dropout launches (claims included) {launches:.3f} ms, "
      f"the rest (two residual epilogues per layer given up, their gradients' extra accumulation) {diff - launches:.3f} ms")
print(json.dumps({"batch": batch, "seq": SEQ, "ms_per_step": {str(p): med[p] for p in med},
                  "rounds_ms": {str(p): ms[p] for p in ms}, "dropout_launch_ms": launches, "difference_ms": diff}))
