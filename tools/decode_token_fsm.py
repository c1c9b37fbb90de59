"""What token-FSM constrained decoding costs on the decode path: tokens/s with `token_fsm` off and on for the 6-layer Llama
at the `bench.py --config decode` shape (V 32000, D 288, 6 heads, F 768, max_seq_len 1024, random weights), greedy and
sampled (temperature 0.8, top_p 0.9).  On: every request has its own machine -- a 16-way `TokenFSM.from_sequences` choice
of 4 .. 12 tokens followed by the end token for good (its own 16 sequences), or, every fourth request, a
`TokenFSM.free_until` machine: free text until a closing token, then a choice.  No stop ids, so that off and on hand out
the same number of tokens:
  generate B=1        the narrow rectangular step, an 8-token prompt;
  ragged B=8          `generate_ragged` over 8 prompts of 1-64 tokens (the narrow per-row step);
  wide B=64 / B=256   `generate_ragged` on the wide step;
  serve               the mix of tools/decode_serve.py: 64 requests through 8 slots.
Tokens/s count the tokens handed out after the prompt pass, with a host read-back per step; off and on alternate in one
process so that clock drift hits both alike, and the medians of `repeats` runs are reported.
usage: python tools/decode_token_fsm.py [new_tokens] [repeats] [all | none | case,case,...] [off | trace]
`off` as the fourth argument: only the off runs, without the keyword -- the form that also runs on a checkout from before
the feature, for the parent comparison (this tool copied into that checkout's tools/).
`trace`: one run per case with `token_fsm` AND the logit edits of tools/decode_logit_edits.py on, nothing timed -- under
`rocprofv3 --kernel-trace --stats -- python tools/decode_token_fsm.py 100 1 generate_B1,ragged_B8,wide_B64,wide_B256 trace`
every step then holds fsm_kernel and logit_edit_kernel side by side over the same B x V logits, told apart by the grid's
second dimension."""
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
if not OFF_ONLY:
    from pydynet_amd.llm.token_fsm import TokenFSM
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
END = V - 1
_made = {}


def machines(n):
    """Per-request machines for n requests (built once per n): a 16-way choice each, every fourth a free-until machine."""
    if n not in _made:
        r = np.random.default_rng(7)
        out = []
        for i in range(n):
            seqs = [r.integers(0, V - 1, int(k)).tolist() for k in r.integers(4, 13, 16)]
            f = TokenFSM.from_sequences(seqs, END)
            out.append(TokenFSM.free_until(int(r.integers(0, V - 1)), f) if i % 4 == 3 else f)
        _made[n] = out
    return dict(token_fsm=_made[n])


def edits(n):
    """The per-request edits of tools/decode_logit_edits.py (the `trace` runs)."""
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


def run(case, kw, on, more=None):
    model = models["on" if on else "off"]
    extra = lambda n: dict(machines(n), **(more(n) if more else {})) if on else {}
    if case == "generate_B1":
        steps, dt = timed(model.generate(rect, 8 + new_tokens + 1, **kw, **extra(1)))
        return steps / dt
    if case == "serve":
        steps, dt = timed(model.serve(serve_prompts, serve_budgets, slots=8, **kw, **extra(64)))
        return (sum(serve_budgets) - 8) / dt                # (the first step's 8 prompt-pass tokens are not timed)
    B = {"ragged_B8": 8, "wide_B64": 64, "wide_B256": 256}[case]
    steps, dt = timed(model.generate_ragged(ragged[:B], new_tokens + 1, **kw, **extra(B)))
    return steps * B / dt


ALL = ("generate_B1", "ragged_B8", "wide_B64", "wide_B256", "serve")
CASES = ALL if len(sys.argv) <= 3 or sys.argv[3] == "all" else () if sys.argv[3] == "none" else tuple(sys.argv[3].split(","))
if TRACE:
    for case in CASES:
        print(f"{case:12s} with token_fsm and logit edits: {run(case, {}, True, edits):9.1f} tokens/s (first run, captures "
              f"included)", flush=True)
    sys.exit(0)
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
print(json.dumps({"tok_s": res, "new_tokens": new_tokens, "repeats": repeats, **({"off_only": True} if OFF_ONLY else {})}))
