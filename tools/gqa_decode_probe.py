"""Decode of a grouped-query Llama at the stories15M shape (vocabulary 32000, dim 288, 6 heads, ffn 768, 6 layers; prompt
64, 200 new tokens, greedy): tokens/s of `Llama.generate` with 6 query heads over 2 and over 1 key/value heads on the
graph-replayed step (csrc/decode_gqa.hip) against the same model on the tape-node path (fast_decode = False: the path every
grouped model decoded on before), and against the multi-head model on the like-for-like five-launch form
(fused_decode = 0) and on its default block form.  The routes alternate in one process; medians of ROUNDS runs with their
spans.  `--trace`: instead, a few steps of the grouped and the multi-head model at max_seq_len 1024 from position ~1000,
batch 8, five-launch form, for a kernel trace (the attention kernels' times; bytes of K/V a step reads are printed).
usage: python tools/gqa_decode_probe.py [--batches 1,8,64,256] [--trace]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pydynet_amd as pdn
from pydynet_amd import hipnp as hp
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama

V, D, H, F, LAYERS, PROMPT, NEW, ROUNDS = 32000, 288, 6, 768, 6, 64, 200, 3


def model(B, kv, max_len):
    Graph.clear()
    np.random.seed(0)
    m = Llama(V, D, H, F, max_len, B, LAYERS, np.float32, n_kv_heads=kv)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    m.to("hip:0")
    m.eval()
    return m


def run(m, ids, n, fast=True, fused=2):
    """Seconds of the n decode steps behind the prompt pass, and the tokens."""
    Llama.fast_decode, Llama.fused_decode = fast, fused
    try:
        gen = m.generate(ids, ids.shape[1] + n + 1)
        toks = [next(gen).numpy()]                        # (the prompt pass and the first token: not timed)
        hp.synchronize()
        t0 = time.perf_counter()
        toks += [t.numpy() for t in gen]                  # (reading a step's token is what a caller does)
        hp.synchronize()
        return time.perf_counter() - t0, np.concatenate(toks, 1)
    finally:
        Llama.fast_decode, Llama.fused_decode = True, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    if args.trace:
        B, T = 8, 1024
        for kv in (None, 2, 1):
            m = model(B, kv, T)
            ids = pdn.Tensor(rng.integers(0, V, (B, 990)), dtype=np.int64, device="hip:0")
            run(m, ids, 24, fused=0)
            G = 1 if kv is None else H // kv
            print(f"Hkv {H // G}: K/V bytes a step's attention reads at position 1000, batch {B}, per layer: "
                  f"{2 * B * (H // G) * 1000 * (D // H) * 4}", flush=True)
        return
    for B in (int(b) for b in args.batches.split(",")):
        ids = pdn.Tensor(rng.integers(0, V, (B, PROMPT)), dtype=np.int64, device="hip:0")
        routes = [(f"Hkv {kv} graph", kv, True, 2) for kv in (2, 1)] + [(f"Hkv {kv} tape-node", kv, False, 2) for kv in (2, 1)]
        routes += [("Hkv 6 five-launch", None, True, 0), ("Hkv 6 default", None, True, 2)]
        models = {kv: model(B, kv, 512) for kv in (2, 1, None)}
        times, toks = {}, {}
        for rnd in range(ROUNDS + 1):                     # (round 0 warms every route up: captures, tables)
            for name, kv, fast, fused in routes:
                n = NEW if fast or rnd else 8             # (the tape-node warm-up needs no 200 steps)
                s, tk = run(models[kv], ids, n, fast, fused)
                if rnd:
                    times.setdefault(name, []).append(B * NEW / s)
                    toks[name] = tk
        for name, ts in times.items():
            print(f"B {B:3d}  {name:18s} {np.median(ts):10.0f} tokens/s  (span {min(ts):.0f} .. {max(ts):.0f})", flush=True)
        for kv in (2, 1):
            same = float((toks[f"Hkv {kv} graph"] == toks[f"Hkv {kv} tape-node"]).mean())
            print(f"B {B:3d}  Hkv {kv}: graph / tape-node {np.median(times[f'Hkv {kv} graph']) / np.median(times[f'Hkv {kv} tape-node']):.2f} x, "
                  f"graph / multi-head five-launch {np.median(times[f'Hkv {kv} graph']) / np.median(times['Hkv 6 five-launch']):.3f}, "
                  f"graph / multi-head default {np.median(times[f'Hkv {kv} graph']) / np.median(times['Hkv 6 default']):.3f}; "
                  f"tokens equal to the tape-node path's: {same:.3f}", flush=True)


if __name__ == "__main__":
    main()
