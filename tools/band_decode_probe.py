"""Decode of a sliding-window Llama at the stories15M shape (vocabulary 32000, dim 288, 6 heads, ffn 768, 6 layers;
max_seq_len 4096, window 256, prompt 64, 200 new tokens, greedy): tokens/s of `Llama.generate` of the windowed multi-head
model and of the windowed model over 2 key/value heads on the graph-replayed step (csrc/decode_band.hip) against the same
model on the tape-node path (fast_decode = False: the path every windowed model decoded on before).  The routes alternate
in one process; medians of ROUNDS runs with their spans.
`--trace`: instead, a few steps at batch 8 for a kernel trace -- the windowed model (window `--window`) from positions
~4000 and ~300, and the unwindowed multi-head model on the five-launch form from ~4000 (pdn_decode_attention_rows_f32 is
its attention under `generate_ragged`, the windowed kernel's like for like); `--case N` runs one of the four alone, so a
trace's per-kernel statistics belong to one position.  `--sweep`: tokens/s at batch 8 near position 4000 under
PDN_DECODE_SPLITS 1 / 2 / 4 / 8, windows 256 and 1024.
usage: python tools/band_decode_probe.py [--batches 1,8,64,256] [--trace [--case N] [--window 256]] [--sweep]"""
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

V, D, H, F, LAYERS, T, PROMPT, NEW, ROUNDS = 32000, 288, 6, 768, 6, 4096, 64, 200, 3


def model(B, kv, window):
    Graph.clear()
    np.random.seed(0)
    m = Llama(V, D, H, F, T, B, LAYERS, np.float32, n_kv_heads=kv, sliding_window=window)
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


def trace(window, case):
    B, rng = 8, np.random.default_rng(0)
    cases = (("windowed", None, window, 4000), ("windowed", None, window, 300), ("windowed Hkv 2", 2, window, 4000),
             ("unwindowed", None, None, 4000))
    for name, kv, w, start in cases if case is None else cases[case:case + 1]:
        m = model(B, kv, w)
        Llama.fused_decode = 0
        try:
            for _ in m.generate_ragged([rng.integers(0, V, start) for _ in range(B)], 24):
                pass
        finally:
            Llama.fused_decode = 2
        hp.synchronize()
        st = m._decode_st
        print(f"{name}: window {w}, positions {start} .. {start + 23}, batch {B}, key ranges {st['ns']}, "
              f"keys a row reads {min(w or T, start)}", flush=True)


def sweep():
    """Tokens/s of 100 steps from position 3900 at batch 8 under PDN_DECODE_SPLITS 1 / 2 / 4 / 8, windows 256 and 1024 (the
    plan reads the variable when it is built and keys on it), alternating, medians of ROUNDS."""
    B, rng = 8, np.random.default_rng(0)
    ids = pdn.Tensor(rng.integers(0, V, (B, 3900)), dtype=np.int64, device="hip:0")
    for w in (256, 1024):
        m, times = model(B, None, w), {}
        for rnd in range(ROUNDS + 1):
            for ns in (1, 2, 4, 8):
                os.environ["PDN_DECODE_SPLITS"] = str(ns)
                s, _ = run(m, ids, 100)
                if rnd:
                    times.setdefault(ns, []).append(B * 100 / s)
        os.environ.pop("PDN_DECODE_SPLITS")
        for ns, ts in times.items():
            print(f"W {w:4d}  key ranges {ns}: {np.median(ts):8.0f} tokens/s  (span {min(ts):.0f} .. {max(ts):.0f})", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--window", type=int, default=256)
    ap.add_argument("--case", type=int, default=None)
    args = ap.parse_args()
    if args.trace:
        return trace(args.window, args.case)
    if args.sweep:
        return sweep()
    rng = np.random.default_rng(0)
    for B in (int(b) for b in args.batches.split(",")):
        ids = pdn.Tensor(rng.integers(0, V, (B, PROMPT)), dtype=np.int64, device="hip:0")
        kvs = (None, 2)
        routes = [(f"Hkv {kv or H} graph", kv, True) for kv in kvs] + [(f"Hkv {kv or H} tape-node", kv, False) for kv in kvs]
        models = {kv: model(B, kv, args.window) for kv in kvs}
        times, toks = {}, {}
        for rnd in range(ROUNDS + 1):                     # (round 0 warms every route up: captures, tables)
            for name, kv, fast in routes:
                n = NEW if fast or rnd else 8             # (the tape-node warm-up needs no 200 steps)
                s, tk = run(models[kv], ids, n, fast)
                if rnd:
                    times.setdefault(name, []).append(B * NEW / s)
                    toks[name] = tk
        for name, ts in times.items():
            print(f"B {B:3d}  {name:18s} {np.median(ts):10.0f} tokens/s  (span {min(ts):.0f} .. {max(ts):.0f})", flush=True)
        for kv in kvs:
            g, t = times[f"Hkv {kv or H} graph"], times[f"Hkv {kv or H} tape-node"]
            same = float((toks[f"Hkv {kv or H} graph"] == toks[f"Hkv {kv or H} tape-node"]).mean())
            print(f"B {B:3d}  Hkv {kv or H}: graph / tape-node {np.median(g) / np.median(t):.2f} x, graph median "
                  f"{'above' if np.median(g) > max(t) else 'NOT above'} the tape-node span; "
                  f"tokens equal to the tape-node path's: {same:.3f}", flush=True)


if __name__ == "__main__":
    main()
