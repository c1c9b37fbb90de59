"""Prefix caching on the decode path (`Llama.serve(prefill_chunk=C, prefix_cache=True)` against the same call without the
cache, in one process): the 6-layer Llama at the `bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768,
max_seq_len 1024, random weights, the seeds of tools/decode_serve.py), N = 64 requests through 8 slots, budgets spread over
8-200 new tokens, three request mixes:
  serve     the mix of tools/decode_serve.py: random prompts of 1-64 tokens, no shared prefixes -- what the cache costs
            when it cannot help;
  system    one shared 48-token system prompt followed by a 1-16-token tail per request;
  turns     four conversations of 16 requests, interleaved; request j of a conversation is request j - 1's prompt plus 8
            new tokens (the first has 8).
Per mix, the cache off and on alternate (clock drift hits them alike): tokens/s (the requests' own tokens over the whole
wall time, a host read-back per step), `prefix_stats`, the number and median time of the steps that carried prompt work.
Medians of `repeats` runs.
usage: python tools/decode_prefix.py [repeats] [C]
       python tools/decode_prefix.py kernel [launches]    only the copy kernel, for a kernel trace: `launches` launches of
            one 64-token copy, then as many of eight 64-token copies, over the model's 12 cache tensors"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import _lib, hipnp as hp
from pydynet_amd.llm.llama import Llama

kernel_only = len(sys.argv) > 1 and sys.argv[1] == "kernel"
repeats = int(sys.argv[1]) if len(sys.argv) > 1 and not kernel_only else 3
CHUNK = int(sys.argv[2]) if len(sys.argv) > 2 and not kernel_only else 64
V, D, H, F, LAYERS, SLOTS, N = 32000, 288, 6, 768, 6, 8, 64
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, SLOTS if not kernel_only else 16, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()

if kernel_only:
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    caches = [c.data for layer in model.layers for c in (layer.attention.cache_k, layer.attention.cache_v)]
    tab = hp.asarray(np.array([c._ptr for c in caches], np.int64))
    L, s = _lib.lib(), hp.stream()
    for n in (1, 8):                                        # rows 8 .. 8 + n - 1 into rows 0 .. n - 1
        dst, src, ln = (hp.asarray(a.astype(np.int32)) for a in (np.arange(n), 8 + np.arange(n), np.full(n, 64)))
        hp.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            L.call("pdn_kv_copy_prefix_rows_f32", tab._ptr, len(caches), caches[0]._strides[0], caches[0].shape[0],
                   64, D, dst._ptr, src._ptr, ln._ptr, n, s)     # (as `serve` calls it: the caches as far as the copies reach)
        hp.synchronize()
        mb = n * 64 * D * 4 * len(caches) / 1e6
        print(f"{n} copies of 64 tokens: {mb:.3f} MB read and as much written per launch; {launches} launches back to back "
              f"{(time.perf_counter() - t0) / launches * 1e6:.1f} us each (host clock)")
    sys.exit(0)

rng = np.random.default_rng(0)
serve_prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, N)]
budgets = [int(n) for n in rng.integers(8, 201, N)]
useful = sum(budgets)
system = rng.integers(0, V, 48)
system_prompts = [np.concatenate([system, rng.integers(0, V, int(n))]) for n in rng.integers(1, 17, N)]
turns = [[rng.integers(0, V, 8)] for _ in range(4)]
for conv in turns:
    for _ in range(15):
        conv.append(np.concatenate([conv[-1], rng.integers(0, V, 8)]))
turn_prompts = [turns[r % 4][r // 4] for r in range(N)]
MIXES = {"serve": serve_prompts, "system": system_prompts, "turns": turn_prompts}


def run(prompts, cache):
    times, work, prev = [], [], np.full(SLOTS, -1)
    kw = {"prefix_cache": True} if cache else {}
    with pdn.no_grad():
        hp.synchronize()
        t0 = t = time.perf_counter()
        for reqs, toks in model.serve(prompts, budgets, slots=SLOTS, prefill_chunk=CHUNK, **kw):
            now = time.perf_counter()
            times.append(now - t)
            # a step with prompt work: a request admitted, or a row that yields nothing while it prefills
            work.append(bool(((reqs >= 0) & ((reqs != prev) | (toks < 0))).any()))
            prev, t = reqs, now
        hp.synchronize()
    return useful / (time.perf_counter() - t0), np.array(times), np.array(work)


out = {"N": N, "slots": SLOTS, "chunk": CHUNK, "tokens": useful}
for mix, prompts in MIXES.items():
    run(prompts, False), run(prompts, True)                 # capture the graphs, warm caches
    res = {False: [], True: []}
    for _ in range(repeats):
        for cache in (False, True):
            tps, times, work = run(prompts, cache)
            plain = times[~work]
            res[cache].append({"tok_s": tps, "steps": len(times), "prompt_steps": int(work.sum()),
                               "prompt_step_median_ms": float(np.median(times[work])) * 1e3,
                               "prompt_step_total_ms": float(times[work].sum()) * 1e3,
                               "plain_step_median_ms": float(np.median(plain)) * 1e3 if plain.size else float("nan")})
    stats = dict(model.prefix_stats)                        # (of the last run with the cache on)
    agg = {c: {k: float(np.median([r[k] for r in runs])) for k in runs[0]} for c, runs in res.items()}
    agg[False]["runs_tok_s"], agg[True]["runs_tok_s"] = ([round(r["tok_s"], 1) for r in res[c]] for c in (False, True))
    ratio = agg[True]["tok_s"] / agg[False]["tok_s"]
    out[mix] = {"off": agg[False], "on": agg[True], "ratio": ratio, "prefix_stats": stats,
                "reused_fraction": stats["reused_tokens"] / stats["prompt_tokens"]}
    for name, a in (("off", agg[False]), ("on", agg[True])):
        print(f"{mix:7s} cache {name:3s}: {a['tok_s']:8.1f} tokens/s  runs {a['runs_tok_s']}; {a['steps']:.0f} steps, "
              f"{a['prompt_steps']:.0f} with prompt work (median {a['prompt_step_median_ms']:.3f} ms, "
              f"{a['prompt_step_total_ms']:.1f} ms in all); plain step median {a['plain_step_median_ms']:.3f} ms")
    print(f"{mix:7s} on / off {ratio:.3f}; {stats}; reused {out[mix]['reused_fraction']:.3f} of the prompt tokens")
print(json.dumps(out))
