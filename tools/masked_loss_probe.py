"""What `ignore_index` costs in the training step: the six-layer Llama's `finetune_step` (V 32000, D 288, 6 heads, F 768),
seq 256, one model and one Adam, three settings alternating in one process:
  none      ignore_index=None: the parent's entry points (pdn_cross_entropy_from_lse_f32, pdn_linear_ce_backward_f32)
  set       ignore_index=-100, no target equals it: pdnl_linear_ce_finish_f32 and pdnl_linear_ce_backward_f32 around the same
            products (+ mce_upstream_kernel, mce_mask_rows_kernel; the finish's two launches replace the two of the loss-from-lse)
  half      ignore_index=-100, half of the targets (at random) equal it
They alternate round by round (clock drift hits them alike); a round is `steps` steps between two events; the figure is the
median of the rounds, the yardstick for `set` and `half` is `none` in the same process.
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/masked_loss_probe.py 1 3) the per-launch times of the
added kernels (names mce_*) stand beside the lm_head products'.
usage: python tools/masked_loss_probe.py [rounds=3] [steps=10] [batch=64]
       python tools/masked_loss_probe.py stats KERNEL_STATS.csv     the mce_* kernels and the lm_head products from the stats csv"""
import json
import os
import sys

if len(sys.argv) > 2 and sys.argv[1] == "stats":
    import csv
    for r in csv.DictReader(open(sys.argv[2])):
        name = r["Name"]
        if any(k in name for k in ("mce_", "ce_rows_from_lse", "ce_reduce", "gemm_outres", "ldw_main", "ldx_", "lmh_")):
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
IGNORE = -100

hp.set_device(0)
rng = np.random.default_rng(1)
ids = pdn.Tensor(rng.integers(0, V, (batch, L)), dtype=np.int64, device="hip:0")
full = rng.integers(0, V, (batch * L,))
half = np.where(rng.random(batch * L) < 0.5, IGNORE, full)
tgt_full = pdn.Tensor(full, dtype=np.int64, device="hip:0")
tgt_half = pdn.Tensor(half, dtype=np.int64, device="hip:0")
MODES = {"none": (tgt_full, None), "set": (tgt_full, IGNORE), "half": (tgt_half, IGNORE)}
Graph.clear()
np.random.seed(0)
m = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)
m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
m.to("hip:0")
opt = Adam(m.parameters(), lr=1e-4)

for tgt, ii in MODES.values():                               # warm up: allocations, workspaces, the chunk tables
    for _ in range(2):
        m.finetune_step(ids, tgt, opt, ignore_index=ii)
ms = {name: [] for name in MODES}
loss = {}
for _ in range(rounds):
    for name, (tgt, ii) in MODES.items():
        hp.synchronize()
        a = hp.Event().record()
        for _ in range(steps):
            loss[name] = m.finetune_step(ids, tgt, opt, ignore_index=ii)
        b = hp.Event().record()
        ms[name].append(a.elapsed_ms(b) / steps)
out = {"batch": batch, "seq": L, "rounds": rounds, "steps": steps, "valid_tokens_half": int((half != IGNORE).sum()), "modes": {}}
base = float(np.median(ms["none"]))
for name in MODES:
    med = float(np.median(ms[name]))
    out["modes"][name] = {"ms_per_step": med, "rounds_ms": [round(x, 3) for x in ms[name]], "over_none": med / base,
                          "loss": loss[name]}
    print(f"{name:5s} {med:8.3f} ms/step  ({med / base:.4f} of none)  rounds {[round(x, 3) for x in ms[name]]}  loss {loss[name]:.4f}")
print(json.dumps(out))
