"""What the penalties cost on the decode path: tokens/s with penalties off and on (repetition 1.3, presence 0.4, frequency
0.2) for the 6-layer Llama at the `bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024,
random weights), greedy and sampled (temperature 0.8, top_p 0.9):
  generate B=1        the narrow rectangular step, an 8-token prompt;
  ragged B=8          `generate_ragged` over 8 prompts of 1-64 tokens (the narrow per-row step);
  wide B=64 / B=256   `generate_ragged` on the wide step;
  serve               the mix of tools/decode_serve.py: 64 requests through 8 slots.
Tokens/s count the tokens handed out after the prompt pass, with a host read-back per step; off and on alternate so that
clock drift hits both alike.  Also the time of back-to-back pdn_penalty_step_f32 launches at B = 1, 8, 64 and 256.
usage: python tools/decode_penalty.py [new_tokens] [repeats] [case,case,...]
(for the kernel's own time run it under `rocprofv3 --kernel-trace --stats -- python tools/decode_penalty.py`)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp, _lib
from pydynet_amd.llm import penalties
from pydynet_amd.llm.llama import Llama

new_tokens = int(sys.argv[1]) if len(sys.argv) > 1 else 100
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 2
V, D, H, F, LAYERS = 32000, 288, 6, 768, 6
PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2)
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=1)
hp.set_device(0)
np.random.seed(0)
# two models with the same weights, one per mode: a model keeps the plan (and graphs) of its last generation, so
# alternating the modes on one model would re-plan and re-capture at every run
models = {}
for mode in ("off", "on"):
    np.random.seed(0)
    m = Llama(V, D, H, F, 1024, 256, LAYERS, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    models[mode] = m.to("hip:0")
    models[mode].eval()
rng = np.random.default_rng(0)
rect = rng.integers(0, V, (1, 8))
ragged = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 256)]
serve_prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 64)]
serve_budgets = [int(n) for n in rng.integers(8, 201, 64)]


def timed(it):
    n, t0 = 0, None
    with pdn.no_grad():
        for tok in it:
            if not isinstance(tok, tuple):                   # (serve hands out host arrays already)
                tok[0].numpy()                              # host read-back per step, as infer.py does
            n += 1
            if n == 1:
                hp.synchronize()
                t0 = time.perf_counter()                    # the prompt pass is not timed
        hp.synchronize()
    return n - 1, time.perf_counter() - t0


def run(case, kw):
    model = models["on" if "repetition_penalty" in kw else "off"]
    if case == "generate_B1":
        steps, dt = timed(model.generate(rect, 8 + new_tokens + 1, **kw))
        return steps / dt
    if case == "serve":
        steps, dt = timed(model.serve(serve_prompts, serve_budgets, slots=8, **kw))
        return (sum(serve_budgets) - 8) / dt                # (the first step's 8 prompt-pass tokens are not timed)
    B = {"ragged_B8": 8, "wide_B64": 64, "wide_B256": 256}[case]
    steps, dt = timed(model.generate_ragged(ragged[:B], new_tokens + 1, **kw))
    return steps * B / dt


CASES = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("generate_B1", "ragged_B8", "wide_B64", "wide_B256", "serve")
res = {}
for case in CASES:
    for mode, skw in (("greedy", {}), ("sampled", SAMPLED)):
        run(case, skw), run(case, {**skw, **PEN})            # capture the graphs, warm caches
        off, on = [], []
        for _ in range(repeats):
            off.append(run(case, skw))
            on.append(run(case, {**skw, **PEN}))
        o, p = float(np.median(off)), float(np.median(on))
        res[f"{case}/{mode}"] = {"off_tok_s": o, "on_tok_s": p, "on_over_off_time": o / p}
        print(f"{case:12s} {mode:7s}: off {o:9.1f} tokens/s   on {p:9.1f} tokens/s   step time x{o / p:.3f}")

# the kernel alone: back-to-back launches of the step's form on (B, V) logits, every row live
L, kern = _lib.lib(), {}
for B in (1, 8, 64, 256):
    logits = hp.asarray((3.0 * np.random.default_rng(B).standard_normal((B, V))).astype(np.float32))
    counts, seen = hp.zeros((B, V), np.int32), hp.zeros((B, -(-V // 32)), np.int32)
    start, pos = hp.zeros((B,), np.int32), hp.asarray(np.full(B, 1 << 30, np.int32))
    ids = hp.asarray(np.random.default_rng(B).integers(0, V, (B, 1)))
    prm = hp.asarray(penalties.params_bytes(1.3, 0.4, 0.2))
    nc = L.query("pdn_penalty_chunks", V)
    cv, ci = hp.empty((B, nc), np.float32), hp.empty((B, nc), np.int32)
    n_launch = 500
    for i in range(n_launch + 20):
        if i == 20:
            hp.synchronize()
            t0 = time.perf_counter()
        L.call("pdn_penalty_step_f32", logits._ptr, V, B, V, prm._ptr, counts._ptr, seen._ptr, start._ptr, ids._ptr,
               pos._ptr, 1, cv._ptr, ci._ptr, hp.stream())
    hp.synchronize()
    kern[B] = (time.perf_counter() - t0) / n_launch * 1e6
    print(f"pdn_penalty_step_f32 B {B:3d}: {kern[B]:7.1f} us/launch back to back (V {V})")
print(json.dumps({"tok_s": res, "penalty_step_us": kern, "new_tokens": new_tokens, "penalties": PEN}))
