"""What sampling costs on the decode path: greedy vs sampled generation (temperature 0.8, top_p 0.9) of the 6-layer Llama
at the `bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, batch 1, 8-token prompt, max_seq_len 1024, random
weights), tokens/s with a host read-back per token, and the time of one pdn_sample_rows_f32 launch on a (1, 32000) row.
The two modes alternate (greedy, sampled, greedy, sampled, ...) so that clock drift hits both alike.
usage: python tools/decode_sampling.py [new_tokens] [repeats]
(for the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/decode_sampling.py`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp, _lib
from pydynet_amd.llm.llama import Llama
from pydynet_amd.llm.sampling import params_buffer

new_tokens = int(sys.argv[1]) if len(sys.argv) > 1 else 200
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
V, D, H, F, LAYERS, PROMPT = 32000, 288, 6, 768, 6, 8
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, 1, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()
ids = np.random.randint(0, V, (1, PROMPT))
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=1)


def run(kw):
    n, t0 = 0, None
    with pdn.no_grad():
        for tok in model.generate(ids, PROMPT + new_tokens + 1, **kw):
            tok[0].numpy()                                  # host read-back per token, as infer.py does
            n += 1
            if n == 1:
                hp.synchronize()
                t0 = time.perf_counter()                    # the prompt pass is not timed
        hp.synchronize()
    return (n - 1) / (time.perf_counter() - t0)


res = {"greedy": [], "sampled": []}
run({}), run(SAMPLED)                                       # capture both graphs, warm caches
for _ in range(repeats):
    res["greedy"].append(run({}))
    res["sampled"].append(run(SAMPLED))

# the kernel alone: back-to-back launches on one logits row (launch rate bounds it from above)
logits = hp.asarray((3.0 * np.random.default_rng(0).standard_normal((1, V))).astype(np.float32))
prm, out = params_buffer(0.8, 0, 0.9, 1), hp.empty((1, 1), np.int64)
L, n_launch = _lib.lib(), 2000
for i in range(n_launch + 50):
    if i == 50:
        hp.synchronize()
        t0 = time.perf_counter()
    L.call("pdn_sample_rows_f32", logits._ptr, V, 1, V, prm._ptr, i, out._ptr, hp.stream())
hp.synchronize()
per_launch_us = (time.perf_counter() - t0) / n_launch * 1e6

g, s = float(np.median(res["greedy"])), float(np.median(res["sampled"]))
print(f"greedy : {g:8.1f} tokens/s  ({1e6 / g:6.1f} us/token)   runs {[round(v) for v in res['greedy']]}")
print(f"sampled: {s:8.1f} tokens/s  ({1e6 / s:6.1f} us/token)   runs {[round(v) for v in res['sampled']]}  (T 0.8, top_p 0.9)")
print(f"sampling adds {1e6 / s - 1e6 / g:.1f} us/token; pdn_sample_rows_f32 back to back: {per_launch_us:.1f} us/launch (B 1, V {V})")
print(json.dumps({"greedy_tok_s": g, "sampled_tok_s": s, "sample_launch_us": per_launch_us, "new_tokens": new_tokens}))
