"""What stop sequences cost on the decode path: tokens/s with `stop_sequences` off and on for the 6-layer Llama at the
`bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights), greedy and sampled
(temperature 0.8, top_p 0.9).  On: every request has its own 4 sequences of 2 .. 8 tokens, made of ids the run without
them never produced -- no row ever stops, so off and on hand out the same tokens and the runs are like for like; what is
measured is the extra launch per replayed step (csrc/stop_seq.hip) and the host matcher that follows it:
  ragged B=8          `generate_ragged` over 8 prompts of 1-64 tokens (the narrow per-row step);
  wide B=64 / B=256   `generate_ragged` on the wide step;
  serve               the mix of tools/decode_serve.py: 64 requests through 8 slots.
Tokens/s count the tokens handed out after the prompt pass, with a host read-back per step; off and on alternate in one
process so that clock drift hits both alike, and the medians of `repeats` runs are reported.
usage: python tools/decode_stop_sequences.py [new_tokens] [repeats] [all | none | case,case,...] [off | trace]
`off` as the fourth argument: only the off runs, without the keyword -- the form that also runs on a checkout from before
the feature, for the parent comparison (this tool copied into that checkout's tools/).
`trace`: one run per case with `stop_sequences`, a `token_fsm` that allows everything AND the logit edits of
tools/decode_logit_edits.py on, nothing timed -- under
`rocprofv3 --kernel-trace --stats -- python tools/decode_stop_sequences.py 100 1 ragged_B8,wide_B64,wide_B256 trace`
every step then holds stop_step_kernel, fsm_kernel and logit_edit_kernel side by side, told apart by their grids."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.llm.llama import Llama

new_tokens = int(sys.argv[1]) if len(sys.argv) > 1 else 100
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
V, D, H, F, LAYERS = 32000, 288, 6, 768, 6
HOW = sys.argv[4] if len(sys.argv) > 4 else ""
OFF_ONLY, TRACE = HOW == "off", HOW == "trace"
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
ragged = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 256)]
serve_prompts = [rng.integers(0, V, int(n)) for n in rng.integers(1, 65, 64)]
serve_budgets = [int(n) for n in rng.integers(8, 201, 64)]


def sequences(n, seen):
    """Per-request stop sequences for n requests: 4 sequences of 2 .. 8 tokens each, of ids not in `seen`."""
    free = np.setdiff1d(np.arange(V), np.fromiter(seen, np.int64, len(seen)))
    r = np.random.default_rng(7)
    return [[r.choice(free, int(k)).tolist() for k in r.integers(2, 9, 4)] for _ in range(n)]


def edits(n):
    """The per-request edits of tools/decode_logit_edits.py and a machine that allows everything (the `trace` runs)."""
    from pydynet_amd.llm.token_fsm import TokenFSM
    r = np.random.default_rng(7)
    bias, allow = [], []
    for i in range(n):
        ids = r.permutation(V)[:64]
        b = {int(t): float(v) for t, v in zip(ids, r.standard_normal(64))}
        b.update({int(t): -np.inf for t in ids[:8]})
        bias.append(b if i % 4 in (0, 2) else None)
        allow.append(np.sort(r.permutation(V)[:V // 2]) if i % 4 in (1, 2) else None)
    return dict(logit_bias=bias, allowed_token_ids=allow, token_fsm=TokenFSM([{0: 0}], 0, [0]))


def timed(it, seen=None):
    n, t0 = 0, None
    with pdn.no_grad():
        for tok in it:
            if isinstance(tok, tuple):                       # (serve hands out host arrays already)
                t = tok[1]
            elif seen is None:
                t = tok[0].numpy()                          # host read-back per step, as infer.py does
            else:
                t = tok.numpy()                             # (every row's token: the ids this run produces)
            if seen is not None:
                seen.update(int(v) for v in np.asarray(t).reshape(-1))
            n += 1
            if n == 1:
                hp.synchronize()
                t0 = time.perf_counter()                    # the prompt pass is not timed
        hp.synchronize()
    return n - 1, time.perf_counter() - t0


def run(case, kw, extra=None, seen=None):
    model = models["off" if extra is None else "on"]
    extra = extra or {}
    if case == "serve":
        steps, dt = timed(model.serve(serve_prompts, serve_budgets, slots=8, **kw, **extra), seen)
        return (sum(serve_budgets) - 8) / dt                # (the first step's 8 prompt-pass tokens are not timed)
    B = {"ragged_B8": 8, "wide_B64": 64, "wide_B256": 256}[case]
    steps, dt = timed(model.generate_ragged(ragged[:B], new_tokens + 1, **kw, **extra), seen)
    return steps * B / dt


ROWS = {"ragged_B8": 8, "wide_B64": 64, "wide_B256": 256, "serve": 64}
ALL = ("ragged_B8", "wide_B64", "wide_B256", "serve")
CASES = ALL if len(sys.argv) <= 3 or sys.argv[3] == "all" else () if sys.argv[3] == "none" else tuple(sys.argv[3].split(","))
if TRACE:
    for case in CASES:
        seen = set()
        run(case, {}, None, seen)
        on = dict(edits(ROWS[case]), stop_sequences=sequences(ROWS[case], seen))
        # (the edits change the tokens: a sequence may now occur and stop a row -- nothing is timed here)
        print(f"{case:12s} with stop_sequences, token_fsm and logit edits: {run(case, {}, on):9.1f} tokens/s (first run, "
              f"captures included)", flush=True)
    sys.exit(0)
res = {}
for case in CASES:
    for mode, skw in (("greedy", {}), ("sampled", SAMPLED)):
        seen = set()
        run(case, skw, None, seen)                                       # capture the graphs, warm caches, see the tokens
        extra = None
        if not OFF_ONLY:
            extra = dict(stop_sequences=sequences(ROWS[case], seen))
            run(case, skw, extra)
        off, on = [], []
        for _ in range(repeats):
            off.append(run(case, skw))
            on.append(off[-1] if OFF_ONLY else run(case, skw, extra))
        o, p = float(np.median(off)), float(np.median(on))
        res[f"{case}/{mode}"] = {"off_tok_s": o, "on_tok_s": p, "on_over_off_time": o / p,
                                 "off_runs": [round(v, 1) for v in off], "on_runs": [round(v, 1) for v in on]}
        print(f"{case:12s} {mode:7s}: off {o:9.1f} tokens/s ({min(off):.1f} .. {max(off):.1f})   on {p:9.1f} tokens/s   "
              f"step time x{o / p:.3f}", flush=True)
print(json.dumps({"tok_s": res, "new_tokens": new_tokens, "repeats": repeats, **({"off_only": True} if OFF_ONLY else {})}))
