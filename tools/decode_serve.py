"""Continuous batching against fixed batches on the decode path: the 6-layer Llama at the `bench.py --config decode` shape
(V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights), N = 64 seeded requests with prompts of 1-64 tokens
and budgets spread over 8-200 new tokens, three ways in one run:
  serve          `Llama.serve(prompts, budgets, slots=8)`: a finished row takes the next request;
  serve_chunked  the same with `prefill_chunk=C` (default 64): prompts fed C tokens per step in the mixed step;
  ragged         `Llama.generate_ragged` over eight batches of 8 requests in order, each run to its longest budget.
Tokens/s count the requests' own tokens (sum of the budgets; no stop ids) over the whole wall time, prompt passes
included, with a host read-back per step.  The two modes alternate so that clock drift hits them alike.
The prefill stall: a serve step that admits requests runs their prompt pass while the other rows wait (a chunked step
feeds prompt tokens); reported as the median and the maximum time of such a step and of a step without prompt work, and
the excess over the median plain step summed over the run.
usage: python tools/decode_serve.py [repeats] [C]"""
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
CHUNK = int(sys.argv[2]) if len(sys.argv) > 2 else 64
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


def run_serve(chunk=None):
    times, admits, prev = [], [], np.full(SLOTS, -1)
    with pdn.no_grad():
        hp.synchronize()
        t0 = t = time.perf_counter()
        for reqs, toks in model.serve(prompts, budgets, slots=SLOTS, prefill_chunk=chunk):
            now = time.perf_counter()
            times.append(now - t)
            # a step with prompt work: a request admitted, or a row that yields nothing while it prefills
            admits.append(bool(((reqs >= 0) & ((reqs != prev) | (toks < 0))).any()))
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


run_serve(), run_serve(CHUNK), run_ragged()                # capture the graphs, warm caches
res = {"serve": [], "serve_chunked": [], "ragged": []}
step_stats = {"serve": [], "serve_chunked": []}
for _ in range(repeats):
    for mode in ("serve", "serve_chunked", "ragged"):
        if mode == "ragged":
            res[mode].append(run_ragged())
            continue
        tps, times, adm = run_serve(CHUNK if mode == "serve_chunked" else None)
        res[mode].append(tps)
        plain = times[~adm][1:]                             # (the first step is the first admission's)
        base = float(np.median(plain))
        step_stats[mode].append({"steps": len(times), "prompt_steps": int(adm.sum()),
                                 "prompt_step_median_ms": float(np.median(times[adm])) * 1e3,
                                 "prompt_step_max_ms": float(times[adm].max()) * 1e3,
                                 "plain_step_median_ms": base * 1e3, "plain_step_max_ms": float(plain.max()) * 1e3,
                                 "stall_ms_per_run": float((times[adm] - base).sum()) * 1e3})
med = {m: float(np.median(v)) for m, v in res.items()}
for m in res:
    print(f"{m:13s}: {med[m]:8.1f} tokens/s   runs {[round(v) for v in res[m]]}")
out = {"tok_s": med, "N": N, "slots": SLOTS, "chunk": CHUNK, "tokens": useful}
for m, runs in step_stats.items():
    agg = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    out[m] = agg
    print(f"{m:13s}: {agg['steps']:.0f} steps, {agg['prompt_steps']:.0f} with prompt work: median / max "
          f"{agg['prompt_step_median_ms']:.3f} / {agg['prompt_step_max_ms']:.3f} ms; without: "
          f"{agg['plain_step_median_ms']:.3f} / {agg['plain_step_max_ms']:.3f} ms; stall {agg['stall_ms_per_run']:.1f} ms "
          f"per run")
print(json.dumps(out))
