"""What gradient clipping and decoupled weight decay cost in the training step: the six-layer Llama's `finetune_step`
(V 32000, D 288, 6 heads, F 768, 24.44 M parameters, all trainable), seq 256, batch 64, with four optimizers in one process:
  Adam()                      the default step: pdn_adam_multi_f32, none of the new entries
  Adam(max_grad_norm=1.0)     + grad_sqnorm_multi_kernel, grad_norm_finalize_kernel; adam_multi_clip_kernel<false>
  AdamW()                     adam_multi_clip_kernel<true>
  AdamW(max_grad_norm=1.0)    all three
Each has a model of its own (same weights, same batch).  They alternate round by round (clock drift hits them alike); a
round is `steps` steps between two events; the figure is the median of the rounds.
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/grad_clip_probe.py 1 3) the per-launch times of the
norm kernel (reads 4 B per parameter: 97.8 MB) and of the two update kernels (28 B per parameter) give their GB/s side by side.
usage: python tools/grad_clip_probe.py [rounds=3] [steps=10] [batch=64]
       python tools/grad_clip_probe.py stats KERNEL_STATS.csv    the table of those kernels from the trace's stats csv:
            average and minimum time per launch and GB/s = parameters x bytes per parameter / average time"""
import json
import os
import sys

if len(sys.argv) > 2 and sys.argv[1] == "stats":
    import csv
    N = 24439712                                                  # parameters of the model below
    for r in csv.DictReader(open(sys.argv[2])):
        name = r["Name"]
        if any(k in name for k in ("grad_sqnorm", "grad_norm_finalize", "adam_multi")):
            avg, per = float(r["AverageNs"]), 4 if "sqnorm" in name else 28
            rate = "" if "finalize" in name else f"{N * per / avg:8.1f} GB/s over {N * per / 1e6:.1f} MB"
            print(f"{name[:60]:60s} calls {r['Calls']:>4s}  avg {avg / 1e3:9.2f} us  min {float(r['MinNs']) / 1e3:9.2f} us  {rate}")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam, AdamW

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 64
V, D, H, F_, L, LAYERS = 32000, 288, 6, 768, 256, 6
MODES = {"Adam()": lambda ps: Adam(ps, lr=1e-4),
         "Adam(max_grad_norm=1.0)": lambda ps: Adam(ps, lr=1e-4, max_grad_norm=1.0),
         "AdamW()": lambda ps: AdamW(ps, lr=1e-4),
         "AdamW(max_grad_norm=1.0)": lambda ps: AdamW(ps, lr=1e-4, max_grad_norm=1.0)}

hp.set_device(0)
rng = np.random.default_rng(1)
ids = pdn.Tensor(rng.integers(0, V, (batch, L)), dtype=np.int64, device="hip:0")
tgt = pdn.Tensor(rng.integers(0, V, (batch * L,)), dtype=np.int64, device="hip:0")
Graph.clear()
runs = {}
for name, make in MODES.items():
    np.random.seed(0)
    m = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    m.to("hip:0")
    opt = make(m.parameters())
    runs[name] = (m, opt)
nparams = sum(p.size for p in runs["Adam()"][0].parameters())

for m, opt in runs.values():                                 # warm up: allocations, workspaces, the chunk tables
    for _ in range(2):
        m.finetune_step(ids, tgt, opt)
ms = {name: [] for name in runs}
loss = {}
for _ in range(rounds):
    for name, (m, opt) in runs.items():
        hp.synchronize()
        a = hp.Event().record()
        for _ in range(steps):
            loss[name] = m.finetune_step(ids, tgt, opt)
        b = hp.Event().record()
        ms[name].append(a.elapsed_ms(b) / steps)
out = {"batch": batch, "seq": L, "parameters": int(nparams), "rounds": rounds, "steps": steps, "modes": {}}
base = float(np.median(ms["Adam()"]))
for name, (m, opt) in runs.items():
    med = float(np.median(ms[name]))
    norm = hp.read_later(opt.last_grad_norm).item() if opt.last_grad_norm is not None else None
    out["modes"][name] = {"ms_per_step": med, "rounds_ms": [round(x, 3) for x in ms[name]], "over_adam": med / base,
                          "last_grad_norm": norm, "skipped_steps": opt.skipped_steps(), "loss": loss[name]}
    print(f"{name:26s} {med:8.3f} ms/step  ({med / base:.4f} of Adam())  rounds {[round(x, 3) for x in ms[name]]}  "
          f"grad norm {norm}  loss {loss[name]:.4f}")
print(json.dumps(out))
