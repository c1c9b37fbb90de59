"""Headline benchmark: training-step samples/s of the 6-layer Llama3 (seq 256) on N MI355X.

    python bench.py --gpus N --steps K --warmup W            (any N: with WORLD_SIZE unset the script starts
                                                              its own N ranks, one process per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
                                                             (an external launcher's RANK / WORLD_SIZE are honoured)

One step = zero_grad -> forward -> cross entropy -> backward -> (bucketed RCCL all-reduce,
overlapped) -> Adam, on synthetic token ids resident in HBM, random-init weights, fp32.
Per-GPU batch is fixed (weak scaling); `--dump-outputs DIR` saves what the last timed step computed (dump_outputs).
Prints ONE compact JSON line (< 4 KB) on rank 0 and writes the
full record (per-family GEMM tables, the other configs, memory) to bench_detail.json, which the line names.  The launcher only has to
provide RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT; this script itself uses no
PyTorch -- device memory, streams, events and RCCL all come from libpdnhip.so.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

V, D, H, F_, L, LAYERS = 32000, 288, 6, 768, 256, 6
FLOP_PER_SAMPLE = 3 * L * (LAYERS * (4 * 2 * D * D + 3 * 2 * D * F_ + 2 * 2 * L * D) + 2 * D * V)   # 24.688e9
PEAK_FP32_MFMA = 157.3e12
# causal attention on 32-row x 32-key tiles: (L/32)(L/32 + 1)/2 of the (L/32)^2 score tiles hold an unmasked entry
_T = L // 32
EXECUTED_FLOP_PER_SAMPLE = FLOP_PER_SAMPLE - 3 * L * LAYERS * (2 * 2 * L * D) * (1.0 - (_T + 1) / (2.0 * _T))


def cpu_baseline(seconds_budget=25.0):
    """CPU numbers next to the GPU line (reported baseline, not the target), on this host's cores:
    `value` = the oracle (NumPy restatement of the reference's op sequence, kind "port") at batch 1;
    `product_numpy_device` = this package's own "cpu" device (fused nodes evaluated with NumPy) at
    batch 1 and 8, as BASELINE.md section 3 lists."""
    from oracle import llama as ollama, nn as onn, tape as otape

    def timed(step, budget, max_steps):
        step()                                          # warm-up (page faults)
        t0, n = time.perf_counter(), 0
        while n < 2 or (time.perf_counter() - t0 < budget and n < max_steps):
            step()
            n += 1
        return n, time.perf_counter() - t0

    otape.reset_tape()
    np.random.seed(0)
    m = ollama.Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)
    m.params["tok_embedding.weight"].value[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    ids, tgt = np.random.randint(0, V, (1, L)), np.random.randint(0, V, (1, L))
    opt = onn.Adam(m.parameters(), lr=1e-4)
    n, dt = timed(lambda: m.finetune_step(ids, tgt, opt), seconds_budget * 0.4, 6)
    out = {"value": n / dt, "unit": "samples/s", "cores": os.cpu_count(), "kind": "port",
           "sample": f"{n} steps of the same model at batch 1 (seq 256), NumPy/BLAS default threads, after 1 warm-up step"}
    del m, opt
    import pydynet_amd as pdn  # noqa: F401
    from pydynet_amd.core.tensor import Graph
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    prod = {}
    for B, share, cap in ((1, 0.2, 6), (8, 0.4, 3)):
        Graph.clear()
        np.random.seed(0)
        pm = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)
        pm.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
        popt = Adam(pm.parameters(), lr=1e-4)
        pids, ptgt = np.random.randint(0, V, (B, L)), np.random.randint(0, V, (B, L))
        n, dt = timed(lambda: pm.finetune_step(pids, ptgt, popt), seconds_budget * share, cap)
        prod[f"batch_{B}"] = {"samples_per_s": B * n / dt, "steps": n}
        del pm, popt
    Graph.clear()
    out["product_numpy_device"] = prod
    return out


# Parity gate (SURVEY 8d "parity gate before timing"): numbers the REAL reference produced for this
# exact model (seed 0, B = 1; tools/gen_golden.py -> tests/golden/llama_full.json, embedded here so the
# gate does not depend on the fixture file travelling with the script).
GATE_LOSS = 11.395865440368652
GATE_GRAD_NORMS = {"lm_head.weight": 1.060440380538923, "tok_embedding.weight": 34.0423977926973,
                   "layers.0.attention.Q.weight": 5.102858180800156, "layers.5.ffn.down.weight": 0.6188517568614766}
GATE_RTOL = 1e-4


COUNTER_SLOTS = ("rowres_chunk", "rowtile_plain", "rowtile_swiglu_fwd", "rowtile_swiglu_bwd", "rowtile_rope", "rowtile_rowmax",
                 "rowres_chunk_epilogue", "attention_p_fwd", "attention_p_bwd", "attention_resident_fwd",
                 "attention_resident_bwd", "attention_stream", "lm_head_dx_sumexp", "lm_head_dw_ce", "outres", "outres_tn",
                 "linear_relu_fwd", "linear_dx_masked", "ce_small", "tiled_swiglu_fwd", "tiled_swiglu_bwd",
                 "conv_quad_fwd", "conv_quad_dgrad", "conv_quad_wgrad")


def kernel_counters(lib, reset=False):
    """Launches per kernel since the last reset, from the library's own counters (include/pdn_hip.h: pdn_kernel_counters)."""
    import ctypes
    buf = (ctypes.c_int64 * len(COUNTER_SLOTS))()
    lib.call("pdn_kernel_counters", buf, len(COUNTER_SLOTS), 1 if reset else 0)
    return dict(zip(COUNTER_SLOTS, (int(v) for v in buf)))


class count_nodes:
    """Counts constructions of the fused tape nodes the timed step is made of (and lowers their row thresholds, so that a
    256-token gate step takes the nodes AND kernels the 65536-token step takes)."""

    def __init__(self):
        from pydynet_amd.core import fused
        self.fused = fused
        self.classes = {"qkv_attention": fused.qkv_attention, "ffn_swiglu": fused.ffn_swiglu,
                        "linear_cross_entropy": fused.linear_cross_entropy}
        self.counts = {k: 0 for k in self.classes}

    def __enter__(self):
        f = self.fused
        self.saved = (f.linear_cross_entropy.min_rows, f.ffn_swiglu.epilogue_min_rows, f.qkv_attention.rope_min_rows)
        f.linear_cross_entropy.min_rows, f.ffn_swiglu.epilogue_min_rows, f.qkv_attention.rope_min_rows = 32, 1, 1
        self.orig = {}
        for name, cls in self.classes.items():
            self.orig[name] = cls.__init__

            def counting(obj, *a, _n=name, _o=cls.__init__, **k):
                self.counts[_n] += 1
                _o(obj, *a, **k)
            cls.__init__ = counting
        return self

    def __exit__(self, *exc):
        f = self.fused
        for name, cls in self.classes.items():
            cls.__init__ = self.orig[name]
        f.linear_cross_entropy.min_rows, f.ffn_swiglu.epilogue_min_rows, f.qkv_attention.rope_min_rows = self.saved
        return False


def require_path(what, nodes, kernels, layers, full_size):
    """Raise unless the step was made of the fused nodes and launched the kernels the timed step is priced on.
    `full_size`: enough tokens for the tile-piece projections (else the same entry points run the chunk kernel)."""
    want_nodes = {"qkv_attention": layers, "ffn_swiglu": layers, "linear_cross_entropy": 1}
    for k, n in want_nodes.items():
        if nodes is not None and nodes.get(k, 0) != n:
            raise SystemExit(f"bench.py {what} FAILED: fused node {k} was built {nodes.get(k, 0)} times, expected {n} "
                             "-- the step fell back to the unfused composition")
    epi = ("rowtile_swiglu_fwd", "rowtile_swiglu_bwd", "rowtile_rope", "rowtile_rowmax") if full_size else ()
    want = {"attention_p_fwd": layers, "attention_p_bwd": layers, "lm_head_dx_sumexp": 1, "lm_head_dw_ce": 1}
    want.update({k: (1 if k == "rowtile_rowmax" else layers) for k in epi})
    for k, n in want.items():
        if kernels.get(k, 0) < n:
            raise SystemExit(f"bench.py {what} FAILED: kernel {k} was launched {kernels.get(k, 0)} times, expected >= {n} "
                             f"(launches per kernel: {kernels})")
    if not full_size:      # the fused-epilogue entry points must have run, on either kernel
        if kernels["rowres_chunk_epilogue"] + sum(kernels[k] for k in COUNTER_SLOTS[2:6]) < 3 * layers + 1:
            raise SystemExit(f"bench.py {what} FAILED: the fused-epilogue projections were not launched ({kernels})")


def parity_gate(model, dev, pdn, lib=None):
    """One forward + backward of the seed-0 model on the reference's seed-0 batch; raises unless the
    loss and the gradient norms match what the reference computed (1e-4 relative)."""
    ids = np.random.randint(0, V, (1, L))               # same RNG stream as the generator: seed 0, model
    tgt = np.random.randint(0, V, (1, L))               # construction, embedding draw, then ids, tgt
    gold = os.path.join(ROOT, "tests", "golden", "llama_full.json")
    norms = dict(GATE_GRAD_NORMS)
    if os.path.exists(gold):
        ref = json.load(open(gold))
        assert abs(ref["losses"][0] - GATE_LOSS) < 1e-9
        norms = {k: ref["grad1_norm"][k] for k in norms}
    model.train(True)
    for p in model.parameters():
        p.zero_grad()
    # the gate must take the nodes the timed steps take: at 256 tokens the model would otherwise use the separate
    # lm_head / cross-entropy nodes (the fused one starts at 32768 tokens, where its kernels fill the chip)
    if lib is None:
        from pydynet_amd import _lib
        lib = _lib.lib()
    kernel_counters(lib, reset=True)
    with count_nodes() as cn:
        loss = model.loss(ids, tgt)
        loss.backward()
    launched = kernel_counters(lib, reset=True)
    require_path("parity gate", cn.counts, launched, LAYERS, full_size=False)
    got = float(loss.item())
    if not abs(got - GATE_LOSS) <= GATE_RTOL * GATE_LOSS:
        raise SystemExit(f"bench.py parity gate FAILED: loss {got!r} != reference {GATE_LOSS!r} (rtol {GATE_RTOL}); "
                         "no throughput number is reported for a path that does not match the reference")
    worst = 0.0
    params = dict(model.named_parameters())
    for name, want in norms.items():
        if want is None:
            continue
        g = params[name].grad.get().astype(np.float64)
        err = abs(float(np.linalg.norm(g)) - want) / want
        worst = max(worst, err)
        if err > GATE_RTOL:
            raise SystemExit(f"bench.py parity gate FAILED: |grad {name}| off by {err:.2e} relative")
    for p in model.parameters():
        p.zero_grad()
    return {"loss": got, "reference_loss": GATE_LOSS, "rel_err": abs(got - GATE_LOSS) / GATE_LOSS,
            "grad_norms_checked": sum(v is not None for v in norms.values()), "worst_grad_norm_rel_err": worst,
            "rtol": GATE_RTOL, "fused_nodes_built": cn.counts, "kernel_launches": {k: v for k, v in launched.items() if v}}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv, timeout=None):
    """`python bench.py --gpus N` with no launcher: start N copies of this script, one per GPU, each with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set (127.0.0.1: the container hostname may not
    resolve), rank 0 on this process's stdout -- its ONE JSON line is the output -- the others' stdout folded into
    stderr.  Returns the worst exit code; if a rank dies the others are terminated (an RCCL peer would hang)."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=port,
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=None if r == 0 else sys.stderr))
    deadline = None if timeout is None else time.monotonic() + timeout
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            rc = rc or code
            if code != 0:                                   # one rank failed: do not leave its peers in a collective
                for q in live:
                    q.terminate()
        if deadline is not None and time.monotonic() > deadline:
            for q in live:
                q.kill()
            return rc or 124
        time.sleep(0.05)
    return rc


def batch_gate(model, ids_np, tgt_np, dev, pdn, lib, rtol=1e-4, want_families=(2, 3, 4)):
    """Parity of the TIMED batch.  The single-sequence step is pinned to the real reference (parity_gate above,
    tests/test_llama_golden.py), but at 256 tokens `pdn_gemm_f32` never reaches the resident-operand kernels the
    timed step spends most of its time in.  Samples are independent and the loss is a mean over tokens
    (llm/llama/model.py:226-252), so one step on B sequences must equal the mean of the B single-sequence steps:
    loss and EVERY gradient tensor are compared (max |diff| <= rtol x the tensor's largest entry).  The embedding
    gradient is a scatter-ASSIGN (tensor.py:937-940: the last occurrence of a token id in the flattened batch
    wins), restated here from the per-sequence gradients in batch order.  Also asserts -- through the library's
    own per-family counters -- that the batched step really ran on the row-resident / output-resident kernels."""
    import ctypes
    from pydynet_amd import hipnp as hp
    from pydynet_amd.core import fused
    B = ids_np.shape[0]
    tgt_np = np.asarray(tgt_np).reshape(B, -1)
    params = dict(model.named_parameters())
    emb_name = "tok_embedding.weight"
    model.train(True)

    def zero():
        for p in params.values():
            p.zero_grad()

    zero()
    lib.call("pdn_gemm_prof_enable", 1)
    kernel_counters(lib, reset=True)
    lossB = model.loss(ids_np, tgt_np.reshape(-1))
    lossB.backward()
    launched = kernel_counters(lib, reset=True)
    ms2, fl2, n2 = (ctypes.c_double * 5)(), (ctypes.c_double * 5)(), (ctypes.c_int64 * 5)()
    lib.call("pdn_gemm_prof_enable", 0)
    lib.call("pdn_gemm_prof_collect_families", ms2, fl2, n2)
    taken = [int(n2[i]) for i in range(5)]
    missing = [i for i in want_families if taken[i] == 0]
    if missing:
        raise SystemExit(f"bench.py batch gate FAILED: GEMM kernel families {missing} were not launched at batch {B} "
                         f"(launches per family {taken})")
    if want_families:                 # (the timed batch: every kernel the roofline block prices must have run)
        require_path("batch gate", None, launched, LAYERS, full_size=True)
    lossB = float(lossB.item())
    with model.lm_head.weight.device:
        gB = {n: p.grad.copy() for n, p in params.items()}
        zero()
        V, D = params[emb_name].shape
        acc_emb = hp.zeros((V, D), np.float32)
        min_rows = fused.linear_cross_entropy.min_rows
        fused.linear_cross_entropy.min_rows = 32            # the node the reference-pinned B = 1 step is pinned with
        losses = []
        try:
            for b in range(B):
                lb = model.loss(ids_np[b:b + 1], tgt_np[b])
                lb.backward()
                losses.append(lb)
                rows = hp.from_numpy(np.unique(ids_np[b]).astype(np.int64))
                eg = params[emb_name].grad
                acc_emb[rows] = eg[rows]                    # later sequences overwrite: last occurrence wins
                eg[rows] = 0.0
        finally:
            fused.linear_cross_entropy.min_rows = min_rows
        loss1 = float(np.mean([float(l.item()) for l in losses]))
        worst, worst_name = 0.0, None
        for n, p in params.items():
            ref = acc_emb if n == emb_name else p.grad
            ref = ref * np.float32(1.0 / B)
            scale = float(abs(ref).max().item())
            err = float(abs(gB[n] - ref).max().item()) / max(scale, 1e-30)
            if err > worst:
                worst, worst_name = err, n
        zero()
    if not abs(lossB - loss1) <= rtol * abs(loss1):
        raise SystemExit(f"bench.py batch gate FAILED: loss at batch {B} = {lossB!r}, mean of the single-sequence "
                         f"losses = {loss1!r}")
    if worst > rtol:
        raise SystemExit(f"bench.py batch gate FAILED: gradient {worst_name} at batch {B} differs from the mean of the "
                         f"single-sequence gradients by {worst:.2e} of its largest entry (rtol {rtol})")
    return {"batch": B, "loss": lossB, "mean_single_sequence_loss": loss1, "loss_rel_err": abs(lossB - loss1) / abs(loss1),
            "grad_tensors_checked": len(params), "worst_grad_rel_err": worst, "worst_grad": worst_name, "rtol": rtol,
            "gemm_family_launches": dict(zip(("tiled", "tn_stream", "rowres", "outres", "outres_tn"), taken)),
            "kernel_launches": {k: v for k, v in launched.items() if v}}


def pmc_traffic(batch=256):
    """HBM bytes per launch from the committed rocprofv3 PMC summary of this same command (FETCH_SIZE x 2 -- the
    gfx950 correction of MI355X_MICROARCH.md -- plus WRITE_SIZE, separate --pmc passes; tools/round_evidence.sh
    regenerates it with tools/pmc_cmd.sh + tools/stamp_pmc.py).  Counters cannot be read from inside the timed run,
    so `traffic` is null when no summary is there.  The newest round's file is taken; `_sha12` identifies it and
    `_stale` says whether the kernel sources have changed since it was collected."""
    import glob
    import hashlib
    # (counter summaries are per launch: only one collected at THIS per-GPU batch describes this run's launches;
    #  `_meta.per_gpu_batch`, 256 for the files of rounds 1-4)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_bench_b256.json")) +
                   glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_bench_default.json")),
                   key=lambda f: os.path.basename(f)[:3])
    path = raw = rows = meta = None
    for cand in reversed(files):
        raw = open(cand, "rb").read()
        rows = json.loads(raw)
        meta = rows.pop("_meta", {})
        if int(meta.get("per_gpu_batch", 256)) == int(batch):
            path = cand
            break
    if path is None:
        return {}
    rel = os.path.relpath(path, ROOT)
    out = {"_source": f"{rel} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, same command)",
           "_sha12": hashlib.sha256(raw).hexdigest()[:12], "_stale": None}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import stamp_pmc
        if meta.get("kernel_sources_sha16"):
            out["_stale"] = meta["kernel_sources_sha16"] != stamp_pmc.sources_sha()
    except Exception:
        pass
    def is_rowres(name):
        return name.startswith("gemm_rowres_kernel") or name.startswith("gemm_rowtile_kernel")

    def is_fused(name):                   # SwiGLU forward / backward, RoPE in the store: EPI 1 / 2 / 3
        n = name.rstrip()
        if name.startswith("gemm_rowres_kernel"):
            return n.endswith((", 1>", ", 2>", ", 3>"))
        if name.startswith("gemm_rowtile_kernel"):          # gemm_rowtile_kernel<BT, EPI, GUARD>
            return any(f", {e}, " in n for e in (1, 2, 3))
        return False

    for fam in ("gemm_f32_mfma_kernel", "gemm_tn_stream_dma_kernel", "row_resident", "gemm_outres_kernel",
                "gemm_outres_tn_kernel", "adam_multi_kernel", "row_resident<EPI>", "rmsnorm_bwd_kernel"):
        n = tot = 0.0
        for name, r in rows.items():
            if fam == "row_resident":
                match = is_rowres(name)                     # the whole template family, fused epilogues included
            elif fam == "row_resident<EPI>":
                match = is_rowres(name) and is_fused(name)
            else:
                match = name.startswith(fam)
            if match and "FETCH_SIZE" in r and "WRITE_SIZE" in r:
                d = r.get("dispatches", 1)
                n += d
                tot += d * (2.0 * r["FETCH_SIZE"] + r["WRITE_SIZE"]) * 1024.0        # counters are in KiB
        if n:
            out[fam] = tot / n
    return out


def hbm_kernels(adam_events, traffic, nparams=0):
    """The HBM-bound kernel of the step, timed live with HIP events on the launch stream INSIDE the timed steps: achieved =
    ALGORITHMIC bytes per launch / average launch duration, against the 8 TB/s HBM3E peak.  Adam: one multi-tensor launch
    reading p, g, m, v and writing p, m, v (28 B per parameter); the event pair brackets `opt.step()` = that one launch
    (rounds 3-5 timed 20 launches back to back after the step and read 126 us where rocprof shows 108 us in the step)."""
    out = {}
    if adam_events and nparams:
        us = 1e3 * sum(a.elapsed_ms(b) for a, b in adam_events) / len(adam_events)
        nbytes = 28.0 * nparams
        out["adam_multi_kernel"] = {"bound": "hbm", "what": "Adam over every parameter in one launch (optim/optimizer.py:160-196)",
                                    "in_step": True, "achieved": nbytes / (us * 1e-6) / 1e9, "peak": 8000.0, "unit": "GB/s",
                                    "frac": nbytes / (us * 1e-6) / 8e12, "algorithmic_bytes_per_launch": nbytes,
                                    "avg_launch_us": us, "launches_timed": len(adam_events),
                                    "traffic": traffic.get("adam_multi_kernel")}
    return out


def other_configs(*release):
    """BASELINE.json configs 2 and 3 (MLP / LeNet at the reference's batch 256 and at a chip-filling batch), the GRU of
    examples/pydynet/ts_prediction.py and KV-cache greedy decode, each a SHORT run of `bench.py --config ...` (same code:
    bench_other.py -- parity gate against the oracle first, then timed steps, roofline of the dominant kernel) inside the
    default run, so that whoever runs the headline command also holds these numbers -- and short runs of the same Llama
    step at another model width (`llama_dim512`: tiled kernel + SwiGLU in its stores) and at 512 positions (`llama_seq512`:
    attention as 256-row block pairs on the persistent kernels).  Not part of `value`; a failure
    here is recorded, never raised (the headline line must still be printed)."""
    import argparse as _ap
    import gc
    import bench_other
    from pydynet_amd.core.tensor import Graph
    del release
    gc.collect()
    res = {}
    runs = (("mlp_b256", "mlp", 256, 200, 20), ("mlp_b65536", "mlp", 65536, 20, 6), ("lenet_b256", "lenet", 256, 200, 20),
            ("lenet_b4096", "lenet", 4096, 50, 5), ("gru", "gru", 0, 100, 10), ("decode", "decode", 0, 200, 20),
            ("transformer", "transformer", 128, 100, 10))
    try:                                                     # (first: before the graph-replayed runs below)
        Graph.clear()
        res["llama_dim512"] = llama_other_width(512, 8, 1536)
    except BaseException as e:
        res["llama_dim512"] = {"error": f"{type(e).__name__}: {e}"}
    gc.collect()
    try:                                                     # the benchmarked width at 512 positions: attention as 256-row
        Graph.clear()                                        # block pairs on the persistent kernels (csrc/attention_blocks.hip)
        res["llama_seq512"] = llama_other_width(288, 6, 768, batch=128, seq=512)
    except BaseException as e:
        res["llama_seq512"] = {"error": f"{type(e).__name__}: {e}"}
    gc.collect()
    try:                                                     # rounds 1-4 quoted the headline at per-GPU batch 256: kept comparable
        Graph.clear()
        res["llama_b256"] = llama_other_width(288, 6, 768, batch=256, seq=256, steps=10, warmup=3)
    except BaseException as e:
        res["llama_b256"] = {"error": f"{type(e).__name__}: {e}"}
    gc.collect()
    try:
        # the DROP-IN formulation: the same model written with plain operators (tests/models_plain_llama.py = what the
        # reference's own llm/llama/model.py does: RoPE as slices + concat, attention as matmul -> softmax -> matmul),
        # beside the fused-node model at the same batch; parity: tests/test_plain_llama.py (reference-generated vectors)
        Graph.clear()
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import plain_llama_bench
        for pb_batch, pb_steps in ((64, 5), (256, 4)):
            r = plain_llama_bench.run(pb_batch, pb_steps)
            res[f"llama_plain_ops_b{pb_batch}"] = {
                "value": r["plain"]["samples_per_s"], "unit": "samples/s", "ms_per_step": r["plain"]["ms_per_step"],
                "model_flops_frac_of_fp32_mfma_peak": r["plain"]["mfma_frac"],
                "fused_model_same_batch": r["fused"], "plain_over_fused": r["plain_over_fused"],
                "kernel_launches_per_step": r["plain"]["kernel_launches_per_step"],
                "config": {"workload": "6-layer Llama3 written with plain operators (drop-in formulation: RoPE by slices + "
                                       "concat, attention as matmul -> softmax -> matmul, recognised link by link and run as "
                                       "one fused attention node), fwd+bwd+Adam, seq 256", "per_gpu_batch": pb_batch}}
    except BaseException as e:
        res["llama_plain_ops_b64"] = {"error": f"{type(e).__name__}: {e}"}
    gc.collect()
    for key, cfg, batch, steps, warmup in runs:
        a = _ap.Namespace(config=cfg, batch=batch, steps=steps, warmup=warmup, no_graph=False, no_cpu_baseline=True, gpus=1)
        try:
            Graph.clear()
            fn = {"mlp": lambda: bench_other.run_train(a, "mlp"), "lenet": lambda: bench_other.run_train(a, "lenet"),
                  "gru": lambda: bench_other.run_gru(a), "decode": lambda: bench_other.run_decode(a),
                  "transformer": lambda: bench_other.run_transformer(a)}[cfg]
            r = fn()
            r.pop("memory", None)
            res[key] = r
        except BaseException as e:                       # (SystemExit of a failed gate included)
            res[key] = {"error": f"{type(e).__name__}: {e}"}
        gc.collect()
    return res


def llama_other_width(dim, heads, ffn, batch=256, seq=256, layers=6, vocab=32000, steps=6, warmup=3):
    """A SHORT run of the same training step at another model width (the reference's constructor is general:
    llm/llama/model.py:153-197): the row-/output-resident kernels do not apply (contraction 288 only), the step runs on the
    tiled kernel with SwiGLU in its stores (`kernel_launches` shows them).  FLOP count: SURVEY 8d's, general form."""
    import numpy as np
    import pydynet_amd as pdn
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    lib = _lib.lib()
    np.random.seed(0)
    m = Llama(vocab, dim, heads, ffn, max(seq, 256), 1, layers, np.float32)
    m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(vocab, dim)).astype(np.float32)
    m.to("hip:0")
    opt = Adam(m.parameters(), lr=1e-4)
    opt.flatten_grads()
    rng = np.random.default_rng(1)
    ids = pdn.Tensor(rng.integers(0, vocab, (batch, seq)), dtype=np.int64, device="hip:0")
    tgt = pdn.Tensor(rng.integers(0, vocab, (batch * seq,)), dtype=np.int64, device="hip:0")
    m.train(True)

    def step():
        opt.zero_grad(); loss = m.loss(ids, tgt); loss.backward(); opt.step(); return loss

    for _ in range(warmup):
        step()
    hp.synchronize()
    kernel_counters(lib, reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    hp.synchronize()
    dt = (time.perf_counter() - t0) / steps
    launched = {k: v / steps for k, v in kernel_counters(lib, reset=True).items() if v}
    flop = 3 * seq * (layers * (4 * 2 * dim * dim + 3 * 2 * dim * ffn + 2 * 2 * seq * dim) + 2 * dim * vocab)
    return {"metric": "training-step samples/sec (6L Llama3 of another width / sequence length)", "value": batch / dt, "unit": "samples/s",
            "ms_per_step": 1e3 * dt, "steps": steps, "warmup": warmup, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"llm/llama 6-layer Llama3, dim {dim}, {heads} heads (hd {dim // heads}), ffn {ffn}, vocab {vocab}, "
                                   f"seq {seq}, fwd+bwd+Adam", "per_gpu_batch": batch, "parallelism": "dp1"},
            "model_flops_frac_of_fp32_mfma_peak": flop * batch / dt / PEAK_FP32_MFMA, "loss": float(loss.item()),
            "kernel_launches_per_step": launched,
            "parity": "tests/test_wide_llama.py: one step of a width-512 model and one of a width-288 model at 512 positions "
                      "against vectors generated from the real reference"}


DETAIL_FILE = "bench_detail.json"
COMPACT_LIMIT = 4096


def write_detail(full):
    """The full record next to the script (`PDN_BENCH_DETAIL` overrides the path; also under gpurun_out/ when that scratch
    directory exists, so that a gpurun call brings it back).  Returns the path the compact line names."""
    override = os.environ.get("PDN_BENCH_DETAIL")
    path = override or os.path.join(ROOT, DETAIL_FILE)
    written = None
    for p in (path, os.path.join(ROOT, "gpurun_out", DETAIL_FILE)):
        if p != path and (override or not os.path.isdir(os.path.dirname(p))):
            continue
        try:
            with open(p, "w") as f:
                json.dump(full, f, indent=1)
            written = written or p
        except OSError:
            pass
    return os.path.relpath(written, ROOT) if written else None


DUMP_LIMIT = 64 * 10 ** 6                                   # bytes --dump-outputs may write, all files together
DUMP_SEED = 0


def dump_outputs(out_dir, loss, params):
    """`--dump-outputs DIR`: what the last timed step handed its caller -- the loss, every gradient the backward pass left
    and every parameter after the Adam update -- as float32 DIR/<name>.npy, so that two builds can be compared output for
    output on the same seeded inputs.  A tensor that does not fit the byte budget is written as a fixed sample of its
    flattened entries: the indices are drawn without replacement (sorted) from default_rng(DUMP_SEED), so they depend on the
    tensor's size only.  Small tensors are written whole; the largest share what is left equally."""
    fetch = {"loss": lambda: np.float32(loss)}
    sizes = {"loss": 1}
    for n, p in params:
        fetch[f"grad.{n}"], fetch[f"param.{n}"] = p.grad.get, p.data.get
        sizes[f"grad.{n}"] = sizes[f"param.{n}"] = int(p.size)
    budget, cap = (DUMP_LIMIT - 256 * len(sizes)) // 4, {}          # (256 bytes: at least one .npy header)
    for i, k in enumerate(sorted(sizes, key=sizes.get)):    # ascending: each takes min(size, a fair share of the rest)
        cap[k] = min(sizes[k], budget // (len(sizes) - i))
        budget -= cap[k]
    os.makedirs(out_dir, exist_ok=True)
    for k in fetch:
        a = np.asarray(fetch[k](), dtype=np.float32)
        if cap[k] < sizes[k]:
            a = a.reshape(-1)[np.sort(np.random.default_rng(DUMP_SEED).choice(sizes[k], cap[k], replace=False))]
        np.save(os.path.join(out_dir, f"{k}.npy"), a)


def _pick(d, keys):
    return None if d is None else {k: d.get(k) for k in keys if k in d}


def compact_line(full, detail_path=None):
    """The ONE stdout line: the contract's keys, the dominant kernel's roofline, the CPU baseline and the two gates as
    scalars, one number per other config.  Everything else lives in `detail` (write_detail)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "model_flops_frac_of_fp32_mfma_peak", "executed_flops_frac",
            "per_rank_samples_per_s", "final_loss")
    out = {k: full[k] for k in keep if k in full}
    roof = full.get("roofline")
    if roof is not None:
        r = _pick(roof, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launches", "avg_launch_us",
                         "time_share_of_step", "algorithmic_flop_per_launch", "traffic_source", "traffic_stale"))
        if isinstance(r.get("traffic_source"), str):
            r["traffic_source"] = r["traffic_source"].split(" ")[0]
        if roof.get("all_gemm"):
            r["all_gemm_frac"] = roof["all_gemm"]["frac"]
            r["all_gemm_time_share"] = roof["all_gemm"]["time_share_of_step"]
        fams = roof.get("other_gemm_families") or {}
        r["other_families_frac"] = {k: round(v["frac"], 4) for k, v in fams.items() if v.get("launches")}
        adam = (roof.get("hbm_bound_kernels") or {}).get("adam_multi_kernel")
        if adam:
            r["adam_hbm"] = _pick(adam, ("achieved", "peak", "unit", "frac", "avg_launch_us", "traffic"))
        out["roofline"] = r
    else:
        out["roofline"] = None
    cb = full.get("cpu_baseline")
    out["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "sample")) if cb else None
    g = full.get("parity_gate")
    out["parity_gate"] = None if g is None else {"rel_err": g["rel_err"], "worst_grad": g["worst_grad_norm_rel_err"],
                                                 "rtol": g["rtol"], "reference_loss": g["reference_loss"]}
    b = full.get("batch_gate")
    out["batch_gate"] = None if b is None else {"batch": b["batch"], "loss_rel_err": b["loss_rel_err"],
                                                "worst_grad_rel_err": b["worst_grad_rel_err"],
                                                "grad_tensors_checked": b["grad_tensors_checked"], "rtol": b["rtol"]}
    if "comm" in full:
        out["comm"] = full["comm"]
    oc = full.get("other_configs")
    if oc:
        brief = {}
        for k, v in oc.items():
            if "error" in v:
                brief[k] = {"error": str(v["error"])[:80]}
            else:
                brief[k] = {"value": round(v["value"], 1), "unit": v.get("unit"), "ms": round(v.get("ms_per_step", 0.0), 4)}
                if "model_flops_frac_of_fp32_mfma_peak" in v:
                    brief[k]["mfma_frac"] = round(v["model_flops_frac_of_fp32_mfma_peak"], 4)
        out["other_configs"] = brief
    out["detail"] = detail_path
    line = json.dumps(out)
    if len(line) >= COMPACT_LIMIT:                          # never let an addition push the headline out of the tail
        for k in ("other_configs", "comm", "per_rank_samples_per_s"):
            if k in out and len(json.dumps(out)) >= COMPACT_LIMIT:
                out[k] = f"see {detail_path}"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=("llama", "mlp", "lenet", "gru", "decode", "transformer"), default="llama",
                    help="llama = the headline line (BASELINE.json configs 4 / 5); mlp / lenet = configs 2 / 3; gru = "
                         "examples/pydynet/ts_prediction.py; decode = KV-cache greedy generation (bench_other.py)")
    ap.add_argument("--batch", type=int, default=int(os.environ.get("PDN_BENCH_BATCH", "0")),
                    help="per-GPU batch (default: 512 for llama (256 in rounds 1-4), 256 for mlp / lenet, 1568 for gru, 1 for decode)")
    ap.add_argument("--no-graph", action="store_true", help="mlp / lenet / transformer: time eager launches instead of hipGraph replay")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gemm-prof", action="store_true")
    ap.add_argument("--no-parity-gate", action="store_true",
                    help="profiling runs only (keeps the batch-1 gate step out of per-kernel counter averages); "
                         "the JSON line then carries parity_gate = null")
    ap.add_argument("--no-batch-gate", action="store_true",
                    help="skip the parity check of the timed batch against the single-sequence path")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short runs of BASELINE configs 2 / 3 (MLP, LeNet), the GRU and greedy decode that the "
                         "default single-GPU line carries in `other_configs`")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps write what the last one computed (loss, gradients, updated parameters) "
                         "as DIR/<name>.npy, at most 64 MB in all (dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.config != "llama":
        ap.error("--dump-outputs is implemented for the llama config only")

    if args.config != "llama":
        import bench_other
        return bench_other.run(args)
    # per-GPU batch: 512 sequences = 131072 token rows = two row blocks per CU for the row- / output-resident kernels (their
    # per-launch costs -- the burst of A rows, the first piece, the last drain -- are paid once per 2 x the work: 81.5 % of the
    # fp32-MFMA peak against 80.0 % at 256, rounds 1-4's default; 1024: 82.0 %); 32 GB of the 288 GB of HBM in use
    args.batch = args.batch or 512
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: this process becomes one (the ranks re-enter main() with RANK / WORLD_SIZE set)
        if os.environ.get("PDN_BENCH_SPAWN_PROBE") != "1":
            from pydynet_amd import cuda as _cuda
            have = _cuda.device_count()
            if have < args.gpus:
                raise SystemExit(f"bench.py: --gpus {args.gpus} but only {have} GPU(s) are visible")
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))
    if os.environ.get("PDN_BENCH_SPAWN_PROBE") == "1":
        # launcher self-test (tests/test_bench_contract_cpu.py): report what this rank was given, touch no GPU
        rec = {k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
        print(json.dumps({"probe": rec, "argv": sys.argv[1:]}), flush=True)
        return

    import ctypes
    from pydynet_amd import hipnp, _lib
    import pydynet_amd as pdn
    from pydynet_amd import distributed as pdist
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    from pydynet_amd.distributed import DataParallel

    local = int(os.environ.get("LOCAL_RANK", "0"))
    lib = _lib.lib()                                        # no CPU fallback: fail loudly
    hipnp.set_device(local)
    # one process per GPU; the communicator is RCCL through the C ABI (no PyTorch anywhere in this script)
    rank, world = pdist.init_process_group("rccl", local) if int(os.environ.get("WORLD_SIZE", "1")) > 1 else (0, 1)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    force_dp = world == 1 and os.environ.get("PDN_BENCH_FORCE_DP") == "1"   # exercise the RCCL path on one GPU
    if force_dp:
        pdist.init_process_group("rccl", local)
    group = pdist.get_group()
    dev = f"hip:{local}"
    B = args.batch

    np.random.seed(0)                                       # identical weights on every rank
    model = Llama(V, D, H, F_, 1024, 1, LAYERS, np.float32)           # (max_batch_size only sizes the unused KV caches)
    model.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
    model.to(dev)
    gate = None if args.no_parity_gate else parity_gate(model, dev, pdn, lib)    # refuses to go on if the path is wrong
    rng = np.random.default_rng(1000 + rank)                # each rank owns its shard of the global batch
    ids_np, tgt_np = rng.integers(0, V, (B, L)), rng.integers(0, V, (B * L,))
    bgate = None
    if not (args.no_parity_gate or args.no_batch_gate) and rank == 0:
        # the kernels of the TIMED batch, against the reference-pinned single-sequence path, on the timed inputs
        bgate = batch_gate(model, ids_np, tgt_np, dev, pdn, lib,
                           want_families=(2, 3, 4) if B * L >= 57344 else ())
    opt = Adam(model.parameters(), lr=1e-4)
    dp = DataParallel(model, opt, always_reduce=force_dp) if (world > 1 or force_dp) else None
    if dp is None:
        opt.flatten_grads()                                 # one flat gradient buffer: zero_grad is a single fill
    ids = pdn.Tensor(ids_np, dtype=np.int64, device=dev)
    tgt = pdn.Tensor(tgt_np, dtype=np.int64, device=dev)
    model.train(True)

    comm_events = []
    adam_events = None

    def step():
        opt.zero_grad()
        loss = model.loss(ids, tgt)
        loss.backward()
        if dp is not None:
            # time the compute stream spends blocked on the gradient all-reduce (= exposed communication)
            e0, e1 = group.exposed_wait_events()
            lib.call("pdn_event_record", e0, hipnp.stream())
            dp.finish()
            lib.call("pdn_event_record", e1, hipnp.stream())
            comm_events.append((e0, e1))
        if adam_events is not None:
            # the optimizer's ONE launch timed where it runs: events on its stream inside the timed step (a loop of
            # back-to-back Adam launches reads 17 % slower than the same kernel behind the backward pass, rocprof agrees)
            e0, e1 = hipnp.Event(), hipnp.Event()
            e0.record()
            opt.step()
            e1.record()
            adam_events.append((e0, e1))
        else:
            opt.step()
        return loss

    def fence():
        if world > 1:
            group.barrier()
        hipnp.synchronize()

    prev = None
    for _ in range(args.warmup):
        prev = step()
    fence()
    for a, b in comm_events:                                # warm-up steps are not part of the exposed-time average
        lib.call("pdn_event_destroy", a)
        lib.call("pdn_event_destroy", b)
    comm_events.clear()
    if not args.no_gemm_prof:
        lib.call("pdn_gemm_prof_enable", 1)
        adam_events = []
    kernel_counters(lib, reset=True)
    losses = []
    t0 = time.perf_counter()
    # every step's loss is read, one step behind and through an event of its own (hipnp.read_later): a blocking copy
    # on the compute stream would wait for the step just queued and start every step on an empty queue
    prev = hipnp.read_later(prev.data) if prev is not None else None
    for _ in range(args.steps):
        cur = hipnp.read_later(step().data)
        if prev is not None:
            losses.append(prev.item())
        prev = cur
    fence()
    dt = time.perf_counter() - t0
    losses.append(prev.item())

    roof = None
    if not args.no_gemm_prof:
        ms2, fl2, n2 = (ctypes.c_double * 5)(), (ctypes.c_double * 5)(), (ctypes.c_int64 * 5)()
        lib.call("pdn_gemm_prof_enable", 0)
        # the projections with a bandwidth pass folded into their store (SwiGLU forward / backward, RoPE) first: they
        # are reported apart -- FLOPs against the MFMA peak AND algorithmic bytes against HBM -- so that the plain
        # row-resident family stays comparable from round to round
        fms, ffl, fby, fn = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
        lib.call("pdn_gemm_prof_collect_fused", ctypes.byref(fms), ctypes.byref(ffl), ctypes.byref(fby), ctypes.byref(fn))
        lib.call("pdn_gemm_prof_collect_families", ms2, fl2, n2)
        tf = lambda f, m: f / (m * 1e-3) / 1e12 if m > 0 else 0.0
        peak = PEAK_FP32_MFMA / 1e12
        traffic = pmc_traffic(B)

        def fam_rec(ms, fl, n, name):
            return {"achieved": tf(fl, ms), "frac": tf(fl, ms) / peak, "launches": n,
                    "avg_launch_us": 1e3 * ms / max(n, 1), "time_share_of_step": ms * 1e-3 / dt,
                    "algorithmic_flop_per_launch": fl / max(n, 1), "traffic": traffic.get(name)}
        # Five GEMM kernel TEMPLATES share the step; the roofline block is that of the template family with the largest
        # time share -- ALL instantiations of a template together (`achieved` = algorithmic 2MNK of its launches /
        # HIP-event time around them, on the launch stream).  The row-resident family = gemm_rowtile_kernel (round 5;
        # gemm_rowres_kernel below its row threshold) incl. the projections with a fused epilogue, which are ALSO shown
        # as a sub-block with their HBM side (`fused_epilogue_gemms`); the other families are reported beside it.
        keys = ("gemm_f32_mfma_kernel", "gemm_tn_stream_dma_kernel", "row_resident", "gemm_outres_kernel",
                "gemm_outres_tn_kernel")
        shown = {"row_resident": "gemm_rowtile_kernel"}
        fams = {}
        for i, k in enumerate(keys):
            ms_, fl_, n_ = ms2[i], fl2[i], n2[i]
            if k == "row_resident":
                ms_, fl_, n_ = ms_ + fms.value, fl_ + ffl.value, n_ + fn.value
            fams[shown.get(k, k)] = fam_rec(ms_, fl_, n_, k)
        dom = max(fams, key=lambda n: fams[n]["time_share_of_step"])
        f0 = fams[dom]
        roof = {"bound": "mfma", "kernel": dom,
                "kernel_family": "all instantiations of the template; gemm_rowtile_kernel = the row-resident family "
                                 "(plain, + SwiGLU forward / backward, + RoPE, + row maxima)",
                "achieved": f0["achieved"], "peak": peak,
                "unit": "TFLOP/s", "frac": f0["frac"], "traffic": f0["traffic"],
                "launches": f0["launches"], "avg_launch_us": f0["avg_launch_us"],
                "time_share_of_step": f0["time_share_of_step"],
                "algorithmic_flop_per_launch": f0["algorithmic_flop_per_launch"],
                "other_gemm_families": {n: fams[n] for n in fams if n != dom},
                "fused_epilogue_gemms": None if fn.value == 0 else {
                    "what": "the row-resident launches with a bandwidth pass in their store: gate|up + SwiGLU forward, "
                            "dh + SwiGLU backward, q|k|v + RoPE (a SUBSET of the gemm_rowtile_kernel family above)",
                    "launches": fn.value, "avg_launch_us": 1e3 * fms.value / fn.value,
                    "achieved": tf(ffl.value, fms.value), "frac": tf(ffl.value, fms.value) / peak, "unit": "TFLOP/s",
                    "hbm_achieved_GBps": fby.value / (fms.value * 1e-3) / 1e9,
                    "hbm_frac": fby.value / (fms.value * 1e-3) / 8e12,
                    "algorithmic_bytes_per_launch": fby.value / fn.value,
                    "traffic": traffic.get("row_resident<EPI>"),
                    "time_share_of_step": fms.value * 1e-3 / dt},
                "all_gemm": {"achieved": tf(sum(fl2) + ffl.value, sum(ms2) + fms.value),
                             "frac": tf(sum(fl2) + ffl.value, sum(ms2) + fms.value) / peak,
                             "time_share_of_step": (sum(ms2) + fms.value) * 1e-3 / dt},
                "kernel_launches_per_step": {k: v / max(args.steps, 1) for k, v in kernel_counters(lib).items() if v},
                "traffic_source": traffic.get("_source"), "traffic_source_sha12": traffic.get("_sha12"),
                "traffic_stale": traffic.get("_stale")}
        roof["hbm_bound_kernels"] = hbm_kernels(adam_events, traffic,
                                                sum(int(p.size) for p in model.parameters())) if rank == 0 else None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, losses[-1], list(model.named_parameters()))
    per_rank = [B * args.steps / dt]
    if world > 1:
        mine = np.zeros((world,), np.float32)
        mine[rank] = dt
        every = hipnp.from_numpy(mine)
        group.all_reduce(every, pdist.SUM)                       # every rank's own wall time, one slot each
        group.wait()
        per_rank = [B * args.steps / float(t) for t in every.get() if t > 0]      # one entry per rank that answered
        dt = group.all_reduce_scalar(dt, pdist.MAX)              # slowest rank's wall time
    value = world * B * args.steps / dt
    out = {
        "metric": "training-step samples/sec (6L Llama3, seq=256)", "value": value, "unit": "samples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "llm/llama 6-layer Llama3 (dim 288, 6 heads, ffn 768, vocab 32000) fwd+bwd+Adam, random init",
                   "seq_len": L, "per_gpu_batch": B, "global_batch": B * world, "parallelism": f"dp{world}"},
        "model_flops_frac_of_fp32_mfma_peak": FLOP_PER_SAMPLE * value / world / PEAK_FP32_MFMA,
        # SURVEY 8d counts the full L x L scores as the reference computes them; the kernels skip the 28 of 64 32 x 32
        # score tiles that are entirely masked: the same rate priced on the FLOPs actually executed
        "executed_flops_frac": EXECUTED_FLOP_PER_SAMPLE * value / world / PEAK_FP32_MFMA,
        "per_rank_samples_per_s": per_rank,
        "final_loss": losses[-1],
        "parity_gate": gate,
        "batch_gate": bgate,
        "roofline": roof,
    }
    if dp is not None:
        exposed = 0.0
        for a, b in comm_events:
            ms_ = ctypes.c_float()
            lib.call("pdn_event_elapsed_ms", a, b, ctypes.byref(ms_))
            exposed += ms_.value / max(len(comm_events), 1)
            lib.call("pdn_event_destroy", a)
            lib.call("pdn_event_destroy", b)
        comm_events.clear()
        if world > 1:
            exposed = group.all_reduce_scalar(exposed, pdist.MAX)
        cap = getattr(group, "channels_cap", None)
        out["comm"] = {"collective": "all-reduce(sum) of flat fp32 gradient buckets, RCCL", "backend": group.backend,
                       "ranks": len(per_rank), "max_channels": int(cap) if cap else None, "buckets": len(dp.buckets),
                       "bucket_MB": [round((hi - lo) * 4 / 1e6, 2) for lo, hi, _, _ in dp.buckets],
                       "payload_MB_per_step": dp.flat.size * 4 / 1e6, "exposed_ms_per_step": exposed,
                       "note": "exposed = compute-stream time blocked in DataParallel.finish() (max over ranks); "
                               "the rest overlaps backward"}
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
    if rank == 0 and world == 1 and not args.no_other_configs and not force_dp:
        # the headline's model, optimizer state and last step go first (their device memory and tape nodes with them;
        # measured: with them alive the width-512 step below ran 141 ms instead of 128)
        model = opt = dp = ids = tgt = prev = cur = loss = step = None
        out["other_configs"] = other_configs()
    # RCCL writes a version banner through C stdio (block-buffered when piped): every rank pushes its
    # own out, then all ranks meet, and only then rank 0 prints -- the JSON record stays the last line
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    if world > 1:
        group.barrier()
    if rank == 0:
        out["memory"] = hipnp.memory_stats()
        # the FULL record (per-family GEMM tables, fused-epilogue and HBM-bound kernels, the other configs, memory) goes
        # to a side file; stdout carries ONE compact line (< 4 KB: the driver keeps an 8 KB tail of stdout)
        print(json.dumps(compact_line(out, write_detail(out))), flush=True)
    if group is not None:
        if world > 1:
            group.barrier()
        pdist.destroy_process_group()


if __name__ == "__main__":
    main()
