"""What label_smoothing and z_loss cost in the training step: the six-layer Llama (V 32000, D 288, 6 heads, F 768), seq 256, one
model and one Adam, five settings alternating in one process:
  mean      zero_grad -> loss() -> backward -> Adam: the scalar node
  rows      the same step on token_losses().mean(): the reduction='none' node (pdnr_* around the same products)
  smooth    loss(label_smoothing=0.1)
  zloss     loss(z_loss=1e-4)
  both      loss(label_smoothing=0.1, z_loss=1e-4)
The last three are the reduction='none' backward under the upstream vector u' plus the pdnz_* launches (kernels zce_*:
weight sums, finish + reduce, coefficients, the dx correction, the uniform column sums and the class-owned column sums).
They alternate round by round (clock drift hits them alike); a round is `steps` steps between two events; the figure is the
median of the rounds.  The yardsticks are `mean` and `rows` in the same process, never the new code itself.
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/smooth_loss_probe.py 1 3 512) the per-launch times of
the added kernels (names zce_*) stand beside the lm_head products' and the rce_* kernels'.
usage: python tools/smooth_loss_probe.py [rounds=3] [steps=10] [batch=64]
       python tools/smooth_loss_probe.py stats KERNEL_STATS.csv     the zce_* / rce_* kernels and the lm_head products from the csv"""
import json
import os
import sys

if len(sys.argv) > 2 and sys.argv[1] == "stats":
    import csv
    for r in csv.DictReader(open(sys.argv[2])):
        name = r["Name"]
        if any(k in name for k in ("zce_", "rce_", "ce_rows_from_lse", "ce_reduce", "gemm_outres", "ldw_main", "ldx_", "lmh_", "adam")):
            print(f"{name[:70]:70s} calls {r['Calls']:>5s}  avg {float(r['AverageNs']) / 1e3:10.2f} us  "
                  f"min {float(r['MinNs']) / 1e3:10.2f} us  total {float(r['TotalDurationNs']) / 1e6:9.3f} ms")
    sys.exit(0)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.optim import Adam

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
batch = int(sys.argv[3]) if len(sys.argv) > 3 else 64
V, D, H, F_, L, LAYERS = 32000, 288, 6, 768, 256, 6

hp.set_device(0)
rng = np.random.default_rng(1)
ids = pdn.Tensor(rng.integers(0, V, (batch, L)), dtype=np.int64, device="hip:0")
tgt = pdn.Tensor(rng.integers(0, V, (batch * L,)), dtype=np.int64, device="hip:0")
Graph.clear()
np.random.seed(0)
m = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)
m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
m.to("hip:0")
m.train(True)
opt = Adam(m.parameters(), lr=1e-4)


KW = {"mean": {}, "smooth": {"label_smoothing": 0.1}, "zloss": {"z_loss": 1e-4}, "both": {"label_smoothing": 0.1, "z_loss": 1e-4}}


def step(mode):
    opt.zero_grad()
    loss = m.token_losses(ids, tgt).mean() if mode == "rows" else m.loss(ids, tgt, **KW[mode])
    loss.backward()
    opt.step()
    return loss


MODES = ("mean", "rows", "smooth", "zloss", "both")
for mode in MODES:                                           # warm up: allocations, workspaces, the chunk tables
    for _ in range(2):
        step(mode).item()
ms = {name: [] for name in MODES}
loss = {}
for _ in range(rounds):
    for name in MODES:
        hp.synchronize()
        a = hp.Event().record()
        for _ in range(steps):
            last = step(name)
        b = hp.Event().record()
        loss[name] = last.item()
        ms[name].append(a.elapsed_ms(b) / steps)
out = {"batch": batch, "seq": L, "rounds": rounds, "steps": steps, "modes": {}}
base, rows_ms = float(np.median(ms["mean"])), float(np.median(ms["rows"]))
for name in MODES:
    med = float(np.median(ms[name]))
    out["modes"][name] = {"ms_per_step": med, "rounds_ms": [round(x, 3) for x in ms[name]], "over_mean": med / base,
                          "over_rows": med / rows_ms, "loss": loss[name]}
    print(f"{name:6s} {med:8.3f} ms/step  ({med / base:.4f} of mean, {med / rows_ms:.4f} of rows)  "
          f"rounds {[round(x, 3) for x in ms[name]]}  loss {loss[name]:.4f}")
print(json.dumps(out))
