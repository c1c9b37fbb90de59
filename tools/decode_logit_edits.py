"""What the logit edits cost on the decode path: tokens/s with the edits off and on for the 6-layer Llama at the
`bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights), greedy and sampled
(temperature 0.8, top_p 0.9).  On: every request has its own edits -- a logit_bias of 64 entries (8 of them bans), an
allowed set of half the vocabulary, both, or neither, cycling over the requests (no stop ids, so that off and on hand out
the same number of tokens; min_new_tokens only adds a test of one more bit word per thread):
  generate B=1        the narrow rectangular step, an 8-token prompt;
  ragged B=8          `generate_ragged` over 8 prompts of 1-64 tokens (the narrow per-row step);
  wide B=64 / B=256   `generate_ragged` on the wide step;
  serve               the mix of tools/decode_serve.py: 64 requests through 8 slots.
Tokens/s count the tokens handed out after the prompt pass, with a host read-back per step; off and on alternate in one
process so that clock drift hits both alike, and the medians of `repeats` runs are reported.  Also the time of
back-to-back pdne_logit_edit_step_f32 and pdn_penalty_step_f32 launches at B = 1, 8, 64 and 256 on the same logits.
usage: python tools/decode_logit_edits.py [new_tokens] [repeats] [all | none | case,case,...] [off]
`off` as the fourth argument: only the off runs, with no keyword of the edits -- the form that also runs on a checkout
from before the edits, for the parent comparison (this tool copied into that checkout's tools/).
(for the kernels' own times run `rocprofv3 --kernel-trace --stats -- python tools/decode_logit_edits.py 100 1 none`: the
trace then holds logit_edit_kernel and penalty_apply_kernel side by side, 520 launches per row count, told apart by the
grid's second dimension)"""
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
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
V, D, H, F, LAYERS = 32000, 288, 6, 768, 6
OFF_ONLY = len(sys.argv) > 4 and sys.argv[4] == "off"
if not OFF_ONLY:
    from pydynet_amd.llm import logit_edits
SAMPLED = dict(temperature=0.8, top_p=0.9, seed=1)
hp.set_device(0)
np.random.seed(0)
# two models with the same weights, one per mode: a model keeps the plan (and graphs) of its last generation, so
# alternating the modes on one model would re-plan and re-capture at every run
models = {}
for mode in ("off",) if OFF_ONLY else ("off", "on"):
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


def edits(n):
    """Per-request edits for n requests: a bias, an allowed set, both, neither, ..."""
    r = np.random.default_rng(7)
    bias, allow = [], []
    for i in range(n):
        ids = r.permutation(V)[:64]
        b = {int(t): float(v) for t, v in zip(ids, r.standard_normal(64))}
        b.update({int(t): -np.inf for t in ids[:8]})
        bias.append(b if i % 4 in (0, 2) else None)
        allow.append(np.sort(r.permutation(V)[:V // 2]) if i % 4 in (1, 2) else None)
    return dict(logit_bias=bias, allowed_token_ids=allow)


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


def run(case, kw, on):
    model = models["on" if on else "off"]
    if case == "generate_B1":
        steps, dt = timed(model.generate(rect, 8 + new_tokens + 1, **kw, **(edits(1) if on else {})))
        return steps / dt
    if case == "serve":
        steps, dt = timed(model.serve(serve_prompts, serve_budgets, slots=8, **kw, **(edits(64) if on else {})))
        return (sum(serve_budgets) - 8) / dt                # (the first step's 8 prompt-pass tokens are not timed)
    B = {"ragged_B8": 8, "wide_B64": 64, "wide_B256": 256}[case]
    steps, dt = timed(model.generate_ragged(ragged[:B], new_tokens + 1, **kw, **(edits(B) if on else {})))
    return steps * B / dt


ALL = ("generate_B1", "ragged_B8", "wide_B64", "wide_B256", "serve")
CASES = ALL if len(sys.argv) <= 3 or sys.argv[3] == "all" else () if sys.argv[3] == "none" else tuple(sys.argv[3].split(","))
res = {}
for case in CASES:
    for mode, skw in (("greedy", {}), ("sampled", SAMPLED)):
        run(case, skw, False), OFF_ONLY or run(case, skw, True)          # capture the graphs, warm caches
        off, on = [], []
        for _ in range(repeats):
            off.append(run(case, skw, False))
            on.append(off[-1] if OFF_ONLY else run(case, skw, True))
        o, p = float(np.median(off)), float(np.median(on))
        res[f"{case}/{mode}"] = {"off_tok_s": o, "on_tok_s": p, "on_over_off_time": o / p,
                                 "off_runs": [round(v, 1) for v in off], "on_runs": [round(v, 1) for v in on]}
        print(f"{case:12s} {mode:7s}: off {o:9.1f} tokens/s ({min(off):.1f} .. {max(off):.1f})   on {p:9.1f} tokens/s   "
              f"step time x{o / p:.3f}", flush=True)

if OFF_ONLY:
    print(json.dumps({"tok_s": res, "new_tokens": new_tokens, "repeats": repeats, "off_only": True}))
    sys.exit(0)
# the kernels alone: back-to-back launches of the step's forms on the same (B, V) logits, every row live
L, kern = _lib.lib(), {}
for B in (1, 8, 64, 256):
    logits = hp.asarray((3.0 * np.random.default_rng(B).standard_normal((B, V))).astype(np.float32))
    spec = logit_edits.check_args(V=V, n=B, **edits(B))
    state = [hp.asarray(a) for a in logit_edits.allow_bits(spec.allow_rows(range(B)), V)
             + logit_edits.bias_tables(spec.bias_rows(range(B)))]
    start, pos = hp.zeros((B,), np.int32), hp.asarray(np.full(B, 1 << 30, np.int32))
    stop = hp.zeros((-(-V // 32),), np.int32)
    eprm = hp.asarray(logit_edits.params_bytes(0))
    counts, seen = hp.zeros((B, V), np.int32), hp.zeros((B, -(-V // 32)), np.int32)
    ids = hp.asarray(np.random.default_rng(B).integers(0, V, (B, 1)))
    pprm = hp.asarray(penalties.params_bytes(1.3, 0.4, 0.2))
    nc = L.query("pdne_logit_edit_chunks", V)
    cv, ci = hp.empty((B, nc), np.float32), hp.empty((B, nc), np.int32)
    calls = {"pdne_logit_edit_step_f32": (logits._ptr, V, B, V, eprm._ptr, *(a._ptr for a in state), start._ptr, pos._ptr,
                                          1, stop._ptr, cv._ptr, ci._ptr, hp.stream()),
             "pdn_penalty_step_f32": (logits._ptr, V, B, V, pprm._ptr, counts._ptr, seen._ptr, start._ptr, ids._ptr,
                                      pos._ptr, 1, cv._ptr, ci._ptr, hp.stream())}
    n_launch = 500
    for name, args in calls.items():
        for i in range(n_launch + 20):
            if i == 20:
                hp.synchronize()
                t0 = time.perf_counter()
            L.call(name, *args)
        hp.synchronize()
        kern[f"{name}/B{B}"] = (time.perf_counter() - t0) / n_launch * 1e6
        print(f"{name:26s} B {B:3d}: {kern[f'{name}/B{B}']:7.1f} us/launch back to back (V {V})", flush=True)
print(json.dumps({"tok_s": res, "step_us": kern, "new_tokens": new_tokens, "repeats": repeats}))
