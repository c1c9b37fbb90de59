"""What reduction='none' costs in the training step: the six-layer Llama (V 32000, D 288, 6 heads, F 768), seq 256, one model
and one Adam, two settings alternating in one process:
  mean      zero_grad -> loss() -> backward -> Adam: the scalar node (pdn_cross_entropy_from_lse_f32, pdn_linear_ce_backward_f32)
  rows      zero_grad -> token_losses().mean() -> backward -> Adam: pdnr_linear_ce_finish_rows_f32 and
            pdnr_linear_ce_backward_rows_f32 around the same products (+ rce_scale_rows_kernel twice: dx in place, the copy of
            x; rce_abs_max_kernel; rce_colsum_part_kernel / rce_colsum_reduce_kernel: the bias gradient's pass over the logits)
They alternate round by round (clock drift hits them alike); a round is `steps` steps between two events; the figure is the
median of the rounds, the yardstick for `rows` is `mean` in the same process.
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/row_loss_probe.py 1 3 512) the per-launch times of the
added kernels (names rce_*) stand beside the lm_head products'.
usage: python tools/row_loss_probe.py [rounds=3] [steps=10] [batch=64]
       python tools/row_loss_probe.py stats KERNEL_STATS.csv     the rce_* kernels and the lm_head products from the stats csv"""
import json
import os
import sys

if len(sys.argv) > 2 and sys.argv[1] == "stats":
    import csv
    for r in csv.DictReader(open(sys.argv[2])):
        name = r["Name"]
        if any(k in name for k in ("rce_", "ce_rows_from_lse", "ce_reduce", "gemm_outres", "ldw_main", "ldx_", "lmh_", "adam")):
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


def step(mode):
    opt.zero_grad()
    loss = m.loss(ids, tgt) if mode == "mean" else m.token_losses(ids, tgt).mean()
    loss.backward()
    opt.step()
    return loss


MODES = ("mean", "rows")
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
base = float(np.median(ms["mean"]))
for name in MODES:
    med = float(np.median(ms[name]))
    out["modes"][name] = {"ms_per_step": med, "rounds_ms": [round(x, 3) for x in ms[name]], "over_mean": med / base,
                          "loss": loss[name]}
    print(f"{name:5s} {med:8.3f} ms/step  ({med / base:.4f} of mean)  rounds {[round(x, 3) for x in ms[name]]}  loss {loss[name]:.4f}")
print(json.dumps(out))
