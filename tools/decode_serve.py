"""Continuous batching against fixed batches on the decode path: the 6-layer Llama at the `bench.py --config decode` shape
(V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights), N = 64 seeded requests with prompts of 1-64 tokens
and budgets spread over 8-200 new tokens, two ways in one run:
  serve   `Llama.serve(prompts, budgets, slots=8)`: a finished row takes the next request;
  ragged  `Llama.generate_ragged` over eight batches of 8 requests in order, each run to its longest budget.
Tokens/s count the requests' own tokens (sum of the budgets; no stop ids) over the whole wall time, prompt passes
included, with a host read-back per step.  The two modes alternate so that clock drift hits them alike.
The prefill stall: a serve step that admits requests runs their prompt pass while the other rows wait; reported as the
median time of such a step minus the median time of a step without admission, and that excess summed over the run.
usage: python tools/decode_serve.py [repeats]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.llm.llama import Llama

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
V, D, H, F, LAYERS, SLOTS, N = 32000, 288, 6, 768, 6, 8, 64
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, SLOTS, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()
rng = np.random.default_rng(0)
prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, N)]
budgets = [int(n) for n in rng.integers(8, 201, N)]
useful = sum(budgets)


def run_serve():
    times, admits, prev = [], [], np.full(SLOTS, -1)
    with pdn.no_grad():
        hp.synchronize()
        t0 = t = time.perf_counter()
        for reqs, toks in model.serve(prompts, budgets, slots=SLOTS):
            now = time.perf_counter()
            times.append(now - t)
            admits.append(bool(((reqs >= 0) & (reqs != prev)).any()))
            prev, t = reqs, now
        hp.synchronize()
    return useful / (time.perf_counter() - t0), np.array(times), np.array(admits)


def run_ragged():
    with pdn.no_grad():
        hp.synchronize()
        t0 = time.perf_counter()
        for i in range(0, N, SLOTS):
            for tok in model.generate_ragged(prompts[i:i + SLOTS], max(budgets[i:i + SLOTS])):
                tok[0].numpy()                              # host read-back per step, as infer.py does
        hp.synchronize()
    return useful / (time.perf_counter() - t0)


run_serve(), run_ragged()                                   # capture the graphs, warm caches
res = {"serve": [], "ragged": []}
stalls, per_adm, steps = [], [], None
for _ in range(repeats):
    tps, times, adm = run_serve()
    res["serve"].append(tps)
    res["ragged"].append(run_ragged())
    base = float(np.median(times[~adm][1:]))                # (the first step is the first admission's)
    per_adm.append(float(np.median(times[adm])) - base)
    stalls.append(float((times[adm] - base).sum()))
    steps = (len(times), int(adm.sum()), base)
med = {m: float(np.median(v)) for m, v in res.items()}
for m in res:
    print(f"{m:6s}: {med[m]:8.1f} tokens/s   runs {[round(v) for v in res[m]]}")
print(f"serve against eight batches of 8: {med['serve'] / med['ragged'] - 1:+.1%}  ({useful} tokens, {N} requests, "
      f"{steps[0]} serve steps, {steps[1]} with an admission)")
print(f"prefill stall: {np.median(per_adm) * 1e3:.3f} ms per admitting step over a {steps[2] * 1e6:.1f} us decode step, "
      f"{np.median(stalls) * 1e3:.1f} ms per run")
print(json.dumps({"serve_tok_s": med["serve"], "ragged_tok_s": med["ragged"], "stall_ms_per_admission":
                  float(np.median(per_adm)) * 1e3, "stall_ms_per_run": float(np.median(stalls)) * 1e3,
                  "decode_step_us": steps[2] * 1e6, "steps": steps[0], "admission_steps": steps[1], "N": N,
                  "slots": SLOTS, "tokens": useful}))
