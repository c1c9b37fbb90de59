"""What a sampling parameter set per request costs on the decode path: tokens/s of a sampled run with one value per
argument (`scalar`: temperature 0.8, top_p 0.9, one seed) and with a table (`table`: every request its own values --
greedy, temperature 0.8, top_k 50, top_p 0.9, min_p 0.05 or another seed, cycling over the requests) for the 6-layer
Llama at the `bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights):
  ragged B=8          `generate_ragged` over 8 prompts of 1-64 tokens (the narrow per-row step);
  wide B=64 / B=256   `generate_ragged` on the wide step;
  serve               the mix of tools/decode_serve.py: 64 requests through 8 slots.
Tokens/s count the tokens handed out after the prompt pass, with a host read-back per step; scalar and table alternate
in one process so that clock drift hits both alike, and the medians of `repeats` runs are reported.  Also the time of
back-to-back launches of the shared and the per-row ticks at B = 8, 64 and 256 on the same logits.
usage: python tools/decode_per_request.py [new_tokens] [repeats] [all | none | case,case,...] [scalar | uniform]
`scalar` as the fourth argument: only the scalar runs, with no new keyword -- the form that also runs on a checkout from
before the table, for the parent comparison (this tool copied into that checkout's tools/).  `uniform`: the table holds
the scalar run's values for every request, so both runs draw the same tokens and the ratio is the cost of the per-row
launches and of the host's block writes alone.
(for the kernels' own times run `rocprofv3 --kernel-trace --stats -- python tools/decode_per_request.py 100 1 none`: the
trace then holds the <.., false> and <.., true> instantiations of the tick kernels side by side)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp, _lib
from pydynet_amd.llm import sampling
from pydynet_amd.llm.llama import Llama

new_tokens = int(sys.argv[1]) if len(sys.argv) > 1 else 100
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
V, D, H, F, LAYERS = 32000, 288, 6, 768, 6
SCALAR_ONLY = len(sys.argv) > 4 and sys.argv[4] == "scalar"
UNIFORM = len(sys.argv) > 4 and sys.argv[4] == "uniform"
SCALAR = dict(temperature=0.8, top_p=0.9, seed=1)
hp.set_device(0)
# two models with the same weights, one per mode: a model keeps the plan (and graphs) of its last generation, so
# alternating the modes on one model would re-plan and re-capture at every run
models = {}
for mode in ("scalar",) if SCALAR_ONLY else ("scalar", "table"):
    np.random.seed(0)
    m = Llama(V, D, H, F, 1024, 256, LAYERS, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    models[mode] = m.to("hip:0")
    models[mode].eval()
rng = np.random.default_rng(0)
ragged = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 256)]
serve_prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 64)]
serve_budgets = [int(n) for n in rng.integers(8, 201, 64)]


def table(n):
    """One value set per request: greedy, T = 0.8, top_k = 50, top_p = 0.9, min_p = 0.05, another seed, ..."""
    if UNIFORM:
        return {k: [v] * n for k, v in SCALAR.items()}
    sets = [dict(temperature=0.0), dict(temperature=0.8), dict(temperature=1.0, top_k=50), dict(temperature=1.0, top_p=0.9),
            dict(temperature=1.0, min_p=0.05), dict(temperature=1.0, seed=7)]
    rows = [dict(dict(temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, seed=1), **sets[i % 6]) for i in range(n)]
    return {k: [r[k] for r in rows] for k in rows[0]}


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


def run(case, tab):
    model = models["table" if tab else "scalar"]
    if case == "serve":
        steps, dt = timed(model.serve(serve_prompts, serve_budgets, slots=8, **(table(64) if tab else SCALAR)))
        return (sum(serve_budgets) - 8) / dt                # (the first step's 8 prompt-pass tokens are not timed)
    B = {"ragged_B8": 8, "wide_B64": 64, "wide_B256": 256}[case]
    steps, dt = timed(model.generate_ragged(ragged[:B], new_tokens + 1, **(table(B) if tab else SCALAR)))
    return steps * B / dt


ALL = ("ragged_B8", "wide_B64", "wide_B256", "serve")
CASES = ALL if len(sys.argv) <= 3 or sys.argv[3] == "all" else () if sys.argv[3] == "none" else tuple(sys.argv[3].split(","))
res = {}
for case in CASES:
    run(case, False), SCALAR_ONLY or run(case, True)                     # capture the graphs, warm caches
    one, tab = [], []
    for _ in range(repeats):
        one.append(run(case, False))
        tab.append(one[-1] if SCALAR_ONLY else run(case, True))
    o, p = float(np.median(one)), float(np.median(tab))
    res[case] = {"scalar_tok_s": o, "table_tok_s": p, "table_over_scalar_time": o / p,
                 "scalar_runs": [round(v, 1) for v in one], "table_runs": [round(v, 1) for v in tab]}
    print(f"{case:10s}: scalar {o:9.1f} tokens/s ({min(one):.1f} .. {max(one):.1f})   table {p:9.1f} tokens/s   "
          f"step time x{o / p:.3f}", flush=True)

if SCALAR_ONLY:
    print(json.dumps({"tok_s": res, "new_tokens": new_tokens, "repeats": repeats, "scalar_only": True}))
    sys.exit(0)
# the ticks alone: back-to-back launches of the shared and the per-row form on the same (B, V) logits, every row live
# (the positions advance by one per launch; nothing stops a row)
L, kern = _lib.lib(), {}
for B in (8, 64, 256):
    logits = hp.asarray((3.0 * np.random.default_rng(B).standard_normal((B, V))).astype(np.float32))
    tab = sampling.check_request_args(n=B, **dict(dict(temperature=1.0, top_k=0, top_p=1.0, seed=0, min_p=0.0), **table(B)))
    shared, blocks = hp.asarray(sampling.params_bytes(0.8, 0, 0.9, 1)), hp.asarray(tab.blocks(range(B)))
    ids, step, arrive = hp.zeros((B, 1), np.int64), hp.zeros((1,), np.int32), hp.zeros((1,), np.int32)
    wide = "_wide" if B > 8 else ""
    n_launch = 500
    for name, prm in ((f"pdn_decode{wide}_sample_tick_rows_f32", shared), (f"pdnq_decode{wide}_sample_tick_rows_f32", blocks)):
        pos = hp.zeros((B,), np.int32)
        cnt = (pos._ptr, step._ptr) + ((arrive._ptr,) if wide else ())
        for i in range(n_launch + 20):
            if i == 20:
                hp.synchronize()
                t0 = time.perf_counter()
            L.call(name, logits._ptr, V, B, V, prm._ptr, ids._ptr, *cnt, None, None, None, 0, 0, None, hp.stream())
        hp.synchronize()
        kern[f"{name}/B{B}"] = (time.perf_counter() - t0) / n_launch * 1e6
        print(f"{name:40s} B {B:3d}: {kern[f'{name}/B{B}']:7.1f} us/launch back to back (V {V})", flush=True)
print(json.dumps({"tok_s": res, "tick_us": kern, "new_tokens": new_tokens, "repeats": repeats}))
