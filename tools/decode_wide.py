"""The wide decode step (csrc/decode_wide.hip) on the stories15M shape (V 32000, D 288, 6 heads, F 768, 6 layers,
max_seq_len 1024, random weights):
  generate   tokens/s of `Llama.generate` at B = 1, 8, 16, 32, 64, 128, 256 (prompt 64, 200 new tokens per row, greedy,
             host read-back of every step's tokens; the prompt pass is outside the timing);
  serve      the request mix of tools/decode_serve.py scaled to 256 requests (prompts of 1-64 tokens, budgets 8-200)
             through 8 and through 64 slots, tokens/s of the requests' own tokens, prompt passes included;
  generic    the generic step at B = 16 (`Llama.wide_decode = False`) for comparison.
Prints one JSON line.  Kernel statistics of the B = 64 step: `python tools/decode_wide.py --one-step 64` under
`rocprofv3 --kernel-trace --stats -- ...`.  That run is not one step alone: it holds the prompt pass (its own kernels),
the two real runs of the graph capture and the replays of the later steps -- 9 executions of the step in all (the
trace's call counts show it) -- so a step's cost is the sum of its launches' per-call averages (5 per layer + 2).
usage: python tools/decode_wide.py [--one-step B]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.llm.llama import Llama

V, D, H, F, LAYERS, MAXB = 32000, 288, 6, 768, 6, 256
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, MAXB, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()


def gen_tps(B, new=200, prompt=64):
    ids = np.random.default_rng(B).integers(0, V, (B, prompt))
    with pdn.no_grad():
        it = model.generate(ids, prompt + new)
        next(it)[0].numpy()                                     # prompt pass + first token: not timed
        hp.synchronize()
        t0 = time.perf_counter()
        n = 0
        for tok in it:
            tok[0].numpy()                                      # host read-back per step
            n += 1
        hp.synchronize()
    return B * n / (time.perf_counter() - t0)


def serve_tps(slots, N=256):
    rng = np.random.default_rng(0)
    prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, N)]
    budgets = [int(n) for n in rng.integers(8, 201, N)]
    with pdn.no_grad():
        hp.synchronize()
        t0 = time.perf_counter()
        for _ in model.serve(prompts, budgets, slots=slots):
            pass
        hp.synchronize()
    return sum(budgets) / (time.perf_counter() - t0)


if len(sys.argv) > 2 and sys.argv[1] == "--one-step":
    B = int(sys.argv[2])
    ids = np.random.default_rng(B).integers(0, V, (B, 64))
    with pdn.no_grad():
        for i, tok in enumerate(model.generate(ids, 64 + 8)):   # captures the step's graph, then replays it
            tok[0].numpy()
        hp.synchronize()
    sys.exit(0)

res = {}
for B in (1, 8, 16, 32, 64, 128, 256):
    gen_tps(B, new=8)                                           # capture the graphs, warm caches
    res[f"generate_B{B}_tok_s"] = round(gen_tps(B), 1)
    print(f"generate B={B:3d}: {res[f'generate_B{B}_tok_s']:10.1f} tokens/s", flush=True)
for slots in (8, 64):
    serve_tps(slots, N=slots + 8)
    res[f"serve_{slots}slots_tok_s"] = round(serve_tps(slots), 1)
    print(f"serve {slots:3d} slots: {res[f'serve_{slots}slots_tok_s']:10.1f} tokens/s", flush=True)
Llama.wide_decode = False
gen_tps(16, new=8)
res["generic_B16_tok_s"] = round(gen_tps(16), 1)
Llama.wide_decode = True
print(f"generic B= 16: {res['generic_B16_tok_s']:10.1f} tokens/s")
print(json.dumps(res))
