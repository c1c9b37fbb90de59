"""Beam search (csrc/beam.hip) against `generate_ragged` at the same number of rows, on the stories15M shape (V 32000,
D 288, 6 heads, F 768, 6 layers, max_seq_len 1024, random weights): B prompts of 64 tokens, 200 new tokens, no stop ids.
  beam_BxW_tok_s     tokens/s of `beam_search(B prompts, 200, W)`: B * W rows x 200 steps over the wall time, prompt
                     pass and backtracking included;
  ragged_R_tok_s     tokens/s of `generate_ragged` over R = B * W prompts, 200 new tokens, host read-back per step.
Prints one JSON line.  Per-launch kernel times: `python tools/decode_beam.py --one B W` under
`rocprofv3 --kernel-trace --stats -- ...` (one beam search of 16 new tokens at B x W rows).
usage: python tools/decode_beam.py [--one B W]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.llm.llama import Llama

V, D, H, F, LAYERS, MAXB, NEW, PROMPT = 32000, 288, 6, 768, 6, 256, 200, 64
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, MAXB, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()


def prompts(n):
    rng = np.random.default_rng(n)
    return [rng.integers(0, V, PROMPT) for _ in range(n)]


def beam_tps(B, W, new=NEW):
    p = prompts(B)
    with pdn.no_grad():
        hp.synchronize()
        t0 = time.perf_counter()
        model.beam_search(p, new, W)
        hp.synchronize()
    return B * W * new / (time.perf_counter() - t0)


def ragged_tps(R, new=NEW):
    p = prompts(R)
    with pdn.no_grad():
        hp.synchronize()
        t0 = time.perf_counter()
        for tok in model.generate_ragged(p, new):
            tok.numpy()
        hp.synchronize()
    return R * new / (time.perf_counter() - t0)


if len(sys.argv) > 3 and sys.argv[1] == "--one":
    B, W = int(sys.argv[2]), int(sys.argv[3])
    beam_tps(B, W, new=16)
    sys.exit(0)

res = {}
for B, W in ((1, 4), (2, 4), (8, 4), (16, 8), (32, 8)):
    beam_tps(B, W, new=8)                                       # capture the graphs, warm caches
    ragged_tps(B * W, new=8)
    res[f"beam_{B}x{W}_tok_s"] = round(beam_tps(B, W), 1)
    res[f"ragged_{B * W}_tok_s"] = round(ragged_tps(B * W), 1)
    print(f"B x W = {B:2d} x {W:2d}: beam {res[f'beam_{B}x{W}_tok_s']:10.1f}  ragged {res[f'ragged_{B * W}_tok_s']:10.1f}"
          " tokens/s", flush=True)
print(json.dumps(res))
