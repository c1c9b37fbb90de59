"""What packing buys a fine-tuning step: the six-layer Llama's `finetune_step` (V 32000, D 288, 6 heads, F 768), seq 256, over
64 documents of seeded lengths uniform in 16..256, in three forms that alternate in one process:
  (a) padded            one document per row, right-padded, targets of the padding = ignore_index  (64 rows)
  (b) packed            the same documents through llm/packing.pack_sequences with segment_ids: the segmented resident
                        attention kernels of include/pdn_segattn.h (counter slot 43)
  (c) packed, no mask   the packed rows with segment_ids=None: WRONG numbers (documents read each other), the same rows on
                        the attention kernels an unsegmented step takes -- (c) against (b) is what the segmented kernels cost
Each form has a model of its own (same weights).  They alternate round by round; a round is `steps` steps between two events;
the figure is the median of the rounds, as ms / step and as real document tokens / s (padding is not counted).
Under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/packed_probe.py 1 3) the per-launch times of the three
SEG kernels stand beside the plain and persistent ones.
usage: python tools/packed_probe.py [rounds=3] [steps=10] [documents=64]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from pydynet_amd.llm.packing import pack_sequences
from pydynet_amd.optim import Adam

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
n_docs = int(sys.argv[3]) if len(sys.argv) > 3 else 64
V, D, H, F_, L, LAYERS = 32000, 288, 6, 768, 256, 6
IGNORE = -100

hp.set_device(0)
rng = np.random.default_rng(1)
docs = [rng.integers(1, V, int(n)) for n in rng.integers(16, L + 1, n_docs)]
tokens = int(sum(d.size for d in docs))
pad_ids = np.zeros((n_docs, L), np.int64)
pad_tgt = np.full((n_docs, L), IGNORE, np.int64)
for r, d in enumerate(docs):
    pad_ids[r, :d.size], pad_tgt[r, :d.size - 1] = d, d[1:]
pk_ids, pk_tgt, pk_seg = pack_sequences(docs, L, pad_id=0, ignore_index=IGNORE)
assert (pk_tgt != IGNORE).sum() == (pad_tgt != IGNORE).sum()


def dev(a, dt=np.int64):
    return pdn.Tensor(a, dtype=dt, device="hip:0")


FORMS = {
    "padded": (dev(pad_ids), dev(pad_tgt.reshape(-1)), None),
    "packed": (dev(pk_ids), dev(pk_tgt.reshape(-1)), hp.asarray(pk_seg)),
    "packed, no mask": (dev(pk_ids), dev(pk_tgt.reshape(-1)), None),
}
Graph.clear()
runs = {}
for name in FORMS:
    np.random.seed(0)
    m = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    m.to("hip:0")
    runs[name] = (m, Adam(m.parameters(), lr=1e-4))


def step(name):
    m, opt = runs[name]
    ids, tgt, seg = FORMS[name]
    return m.finetune_step(ids, tgt, opt, ignore_index=IGNORE, segment_ids=seg)


for name in runs:                                            # warm up: allocations, workspaces, the chunk tables
    for _ in range(2):
        step(name)
ms = {name: [] for name in runs}
loss = {}
for _ in range(rounds):
    for name in runs:
        hp.synchronize()
        a = hp.Event().record()
        for _ in range(steps):
            loss[name] = step(name)
        b = hp.Event().record()
        ms[name].append(a.elapsed_ms(b) / steps)
hp.check_index_errors()
out = {"documents": n_docs, "seq": L, "document_tokens": tokens, "padded_rows": n_docs, "packed_rows": int(pk_ids.shape[0]),
       "padding_share_padded": 1.0 - tokens / (n_docs * L), "padding_share_packed": 1.0 - tokens / pk_ids.size,
       "rounds": rounds, "steps": steps, "forms": {}}
print(f"{n_docs} documents, {tokens} tokens: {n_docs} padded rows ({out['padding_share_padded']:.1%} padding), "
      f"{pk_ids.shape[0]} packed rows ({out['padding_share_packed']:.1%} padding)")
for name in runs:
    med = float(np.median(ms[name]))
    out["forms"][name] = {"ms_per_step": med, "rounds_ms": [round(x, 3) for x in ms[name]],
                          "document_tokens_per_s": tokens / med * 1e3, "loss": loss[name]}
    print(f"{name:16s} {med:8.3f} ms/step  {tokens / med * 1e3:12.0f} document tokens/s  rounds {[round(x, 3) for x in ms[name]]}  "
          f"loss {loss[name]:.4f}")
print(json.dumps(out))
