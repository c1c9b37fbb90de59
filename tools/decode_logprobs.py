"""What log-probabilities cost on the decode path: tokens/s with logprobs off, n = 0, n = 5 and n = 20 for the 6-layer
Llama at the `bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights), greedy
and sampled (temperature 0.8, top_p 0.9):
  generate_B1 / generate_B8   the narrow rectangular step, 8-token prompts;
  wide_B64 / wide_B256        `generate_ragged` on the wide step, prompts of 1-64 tokens;
  serve / serve_chunked       the mix of tools/decode_serve.py: 64 requests through 8 slots (chunk 64).
Tokens/s count the tokens handed out after the prompt pass, with a host read-back per step; the modes alternate so that
clock drift hits them alike.  Also the time of back-to-back pdn_logprobs_rows_f32 calls at B = 1, 8, 64 and 256.
usage: python tools/decode_logprobs.py [new_tokens] [repeats] [case,case,...]
(for the kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/decode_logprobs.py`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp, _lib
from pydynet_amd.llm.llama import Llama

new_tokens = int(sys.argv[1]) if len(sys.argv) > 1 else 100
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 2
V, D, H, F, LAYERS = 32000, 288, 6, 768, 6
MODES = (None, 0, 5, 20)
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=1)
hp.set_device(0)
# one model per mode, same weights: a model keeps the plan (and graphs) of its last generation
models = {}
for n in MODES:
    np.random.seed(0)
    m = Llama(V, D, H, F, 1024, 256, LAYERS, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    models[n] = m.to("hip:0")
    models[n].eval()
rng = np.random.default_rng(0)
rect = {B: rng.integers(0, V, (B, 8)) for B in (1, 8)}
ragged = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 256)]
serve_prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 64)]
serve_budgets = [int(n) for n in rng.integers(8, 201, 64)]


def timed(it):
    k, t0 = 0, None
    with pdn.no_grad():
        for out in it:
            tok = out[0] if isinstance(out, tuple) else out
            if hasattr(tok, "numpy"):
                tok.numpy()                                 # host read-back per step, as infer.py does
            k += 1
            if k == 1:
                hp.synchronize()
                t0 = time.perf_counter()                    # the prompt pass is not timed
        hp.synchronize()
    return k - 1, time.perf_counter() - t0


def run(case, n, kw):
    model = models[n]
    if n is not None:
        kw = dict(kw, logprobs=n)
    if case.startswith("generate_B"):
        B = int(case[len("generate_B"):])
        steps, dt = timed(model.generate(rect[B], 8 + new_tokens + 1, **kw))
        return steps * B / dt
    if case.startswith("serve"):
        chunk = 64 if case == "serve_chunked" else None
        steps, dt = timed(model.serve(serve_prompts, serve_budgets, slots=8, prefill_chunk=chunk, **kw))
        return (sum(serve_budgets) - 8) / dt
    B = {"wide_B64": 64, "wide_B256": 256}[case]
    steps, dt = timed(model.generate_ragged(ragged[:B], new_tokens + 1, **kw))
    return steps * B / dt


CASES = (tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else
         ("generate_B1", "generate_B8", "wide_B64", "wide_B256", "serve", "serve_chunked"))
res = {}
for case in CASES:
    for mode, skw in (("greedy", {}), ("sampled", SAMPLED)):
        for n in MODES:
            run(case, n, skw)                               # capture the graphs, warm caches
        got = {n: [] for n in MODES}
        for _ in range(repeats):
            for n in MODES:
                got[n].append(run(case, n, skw))
        med = {n: float(np.median(v)) for n, v in got.items()}
        res[f"{case}/{mode}"] = {("off" if n is None else f"n{n}"): v for n, v in med.items()}
        off = med[None]
        print(f"{case:14s} {mode:7s}: off {off:9.1f} tok/s  " +
              "  ".join(f"n={n}: {med[n]:9.1f} (x{off / med[n]:.3f})" for n in MODES[1:]))

# the standalone entry alone: back-to-back calls on (B, V) logits, every row live
L, kern = _lib.lib(), {}
for B in (1, 8, 64, 256):
    logits = hp.asarray((3.0 * np.random.default_rng(B).standard_normal((B, V))).astype(np.float32))
    toks = hp.asarray(np.random.default_rng(B).integers(0, V, B))
    for n in (0, 5, 20):
        work = hp.zeros((L.query("pdn_logprobs_work_bytes", B, V, n) // 8 + 2,), np.int64)
        tok, ids, top = hp.empty((B,), np.float32), hp.empty((B, max(n, 1)), np.int64), hp.empty((B, max(n, 1)), np.float32)
        n_launch = 300
        for i in range(n_launch + 20):
            if i == 20:
                hp.synchronize()
                t0 = time.perf_counter()
            L.call("pdn_logprobs_rows_f32", logits._ptr, V, B, V, n, toks._ptr, tok._ptr, ids._ptr, top._ptr, work._ptr,
                   hp.stream())
        hp.synchronize()
        kern[f"B{B}/n{n}"] = (time.perf_counter() - t0) / n_launch * 1e6
        print(f"pdn_logprobs_rows_f32 B {B:3d} n {n:2d}: {kern[f'B{B}/n{n}']:7.1f} us/call back to back (V {V})")
print(json.dumps({"tok_s": res, "rows_us": kern, "new_tokens": new_tokens}))
