"""Prompt-lookup speculative decoding (csrc/speculative.hip, `generate_ragged(speculate=k)`) on the stories15M shape
(V 32000, D 288, 6 heads, F 768, 6 layers, max_seq_len 1024, random weights, set up as in tools/decode_wide.py).
For B = 1 and 8, k in {0, 2, 4, 8}, 200 new tokens per row and two prompt mixes:
  repetitive  a 16-token random phrase repeated 4 times (64 tokens);
  random      64 random tokens;
greedy, plus one sampled line (temperature 0.8, top-p 0.9, repetitive mix, B = 1, k = 4).  Each line reports tokens/s
(median of 3 runs; host clock around synchronised work, the prompt pass outside it), `passes`, the draft tokens fed
(`drafted`) and accepted (`accepted`), the acceptance rate (accepted / drafted; null when nothing was drafted), tokens
per pass, and whether its tokens equal those of the k = 0 line (`same_tokens_as_k0`).  k = 0 is the plain ragged decode
(its passes: one per step after the prompt pass).  Prints one JSON line.
`python tools/decode_speculative.py --one-step B K` runs one generation at B rows with speculate=K, for
`rocprofv3 --kernel-trace --stats -- python tools/decode_speculative.py --one-step 1 4`."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.llm.llama import Llama

V, D, H, F, LAYERS, MAXB, NEW = 32000, 288, 6, 768, 6, 8, 200
hp.set_device(0)
np.random.seed(0)
model = Llama(V, D, H, F, 1024, MAXB, LAYERS, np.float32)
model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
model = model.to("hip:0")
model.eval()


def prompts(mix, B):
    rng = np.random.default_rng(B)
    if mix == "repetitive":
        return [np.tile(rng.integers(0, V, 16), 4) for _ in range(B)]
    return [rng.integers(0, V, 64) for _ in range(B)]


def run(mix, B, k, **kw):
    with pdn.no_grad():
        it = model.generate_ragged(prompts(mix, B), NEW, speculate=k, **kw)
        next(it).numpy()                                        # prompt pass + first token: not timed
        hp.synchronize()
        t0 = time.perf_counter()
        toks = [tok.numpy().reshape(-1).copy() for tok in it]  # host read-back per step
        hp.synchronize()
        dt = time.perf_counter() - t0
    n = int(sum((t >= 0).sum() for t in toks))
    c = dict(model.last_speculation) if k else {"passes": NEW - 1, "drafted": 0, "accepted": 0, "tokens": n}
    return n / dt, c, np.stack(toks, 1)


def line(mix, B, k, **kw):
    runs = [run(mix, B, k, **kw) for _ in range(3)]
    c = runs[-1][1]
    return {"mix": mix, "B": B, "k": k, "sampled": bool(kw), "tok_s": round(statistics.median(r[0] for r in runs), 1),
            "tokens": runs[-1][2],
            "passes": c["passes"], "drafted": c["drafted"], "accepted": c["accepted"],
            "accept_rate": round(c["accepted"] / c["drafted"], 3) if c["drafted"] else None,
            "tokens_per_pass": round(c["tokens"] / max(c["passes"], 1), 3)}


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one-step":
        B, k = int(sys.argv[2]), int(sys.argv[3])
        run("repetitive", B, k)
        sys.exit(0)
    out = [line(mix, B, k) for mix in ("repetitive", "random") for B in (1, 8) for k in (0, 2, 4, 8)]
    out.append(line("repetitive", 1, 4, temperature=0.8, top_p=0.9, seed=1))
    out.append(line("repetitive", 1, 0, temperature=0.8, top_p=0.9, seed=1))
    # each k > 0 line against the k = 0 line of its mix, B and sampling: the same streams up to fp32 near-ties
    base = {(r["mix"], r["B"], r["sampled"]): r["tokens"] for r in out if r["k"] == 0}
    for r in out:
        t = r.pop("tokens")
        r["same_tokens_as_k0"] = bool(np.array_equal(t, base[(r["mix"], r["B"], r["sampled"])]))
    for r in out:
        print(r, file=sys.stderr)
    print(json.dumps({"speculative": out}))
