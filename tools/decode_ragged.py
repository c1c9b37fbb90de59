"""What a position per row costs on the decode path: generation of the 6-layer Llama at the `bench.py --config decode`
shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights) at batch 8, three ways in one run:
  rect    `generate` on an (8, L) prompt (every row at the same position);
  equal   `generate_ragged` on the same 8 prompts of length L;
  spread  `generate_ragged` on 8 prompts with lengths spread over 1 .. L.
Tokens/s count every row's tokens (8 per step), with a host read-back per step; the prompt pass is not timed.  The
three modes alternate (rect, equal, spread, rect, ...) so that clock drift hits them alike.
usage: python tools/decode_ragged.py [new_tokens] [repeats] [L]
(for the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/decode_ragged.py`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.llm.llama import Llama

new_tokens = int(sys.argv[1]) if len(sys.argv) > 1 else 200
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
PROMPT = int(sys.argv[3]) if len(sys.argv) > 3 else 64
V, D, H, F, LAYERS, B = 32000, 288, 6, 768, 6, 8
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, B, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()
ids = np.random.randint(0, V, (B, PROMPT))
spread = [ids[b, :n] for b, n in enumerate(np.linspace(1, PROMPT, B).astype(int))]


def run(mode):
    it = {"rect": lambda: model.generate(ids, PROMPT + new_tokens + 1),
          "equal": lambda: model.generate_ragged(list(ids), new_tokens + 1),
          "spread": lambda: model.generate_ragged(spread, new_tokens + 1)}[mode]()
    n, t0 = 0, None
    with pdn.no_grad():
        for tok in it:
            tok[0].numpy()                                  # host read-back per step, as infer.py does
            n += 1
            if n == 1:
                hp.synchronize()
                t0 = time.perf_counter()
        hp.synchronize()
    return B * (n - 1) / (time.perf_counter() - t0)


modes = ("rect", "equal", "spread")
res = {m: [] for m in modes}
for m in modes:
    run(m)                                                  # capture the graphs, warm caches
for _ in range(repeats):
    for m in modes:
        res[m].append(run(m))
med = {m: float(np.median(res[m])) for m in modes}
for m in modes:
    print(f"{m:6s}: {med[m]:8.1f} tokens/s  ({B * 1e6 / med[m]:6.1f} us/step)   runs {[round(v) for v in res[m]]}")
print(f"per-row positions: equal {med['equal'] / med['rect'] - 1:+.1%}, spread {med['spread'] / med['rect'] - 1:+.1%} "
      f"against rect (B {B}, prompt {PROMPT}, {new_tokens} new tokens)")
print(json.dumps({f"{m}_tok_s": med[m] for m in modes} | {"B": B, "prompt": PROMPT, "new_tokens": new_tokens}))
