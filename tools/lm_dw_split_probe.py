"""lm_head weight gradient with the cross-entropy gradient formed inside: the fp32 MFMA kernel (csrc/gemm_outres.hip,
gemm_outres_tn_kernel<.., CE>) against the split-fp16 kernel (csrc/lm_head_dw_split.hip: the passes over x of
csrc/split_tn_planes.hip and the product), and the split kernel's timing ablations (PDN_LMHEAD_DW_SPLIT_ABLATE: 1 = constant planes, no logits read -- MFMA
+ LDS only; 2 = the logits fetched once -- no HBM stream, the split arithmetic stays).  Every figure is one call of
pdn_linear_ce_backward_f32 with dx = NULL and includes the two slab reductions (dW and dbias), which both kernels share;
the fp32 kernel is selected by the workspace size (include/pdn_hip.h).  The library reads the ablation switch once, so
every variant runs in a child process of its own, one after the other; a child that fails ends the probe.
usage: python tools/lm_dw_split_probe.py [tokens=131072] [vocab=32000]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 288


def child(T, V):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pydynet_amd import hipnp as hp, _lib
    hp.set_device(0)
    L = _lib.lib()
    ab = os.environ.get("PDN_LMHEAD_DW_SPLIT_ABLATE", "0")
    rng = np.random.default_rng(0)
    x = hp.from_numpy(rng.standard_normal((T, K), dtype=np.float32))
    w = hp.from_numpy((0.05 * rng.standard_normal((K, V))).astype(np.float32))
    tg = hp.from_numpy(rng.integers(0, V, T).astype(np.int64))
    parts = L.query("pdn_linear_rowmax_parts", T, V, K)
    logits, mx = hp.empty((T, V)), hp.empty((parts * T,))
    L.call("pdn_linear_rowmax_fwd_f32", x._ptr, w._ptr, None, logits._ptr, mx._ptr, T, V, K, K, V, V, hp.stream())
    dx, lse = hp.empty((T, K)), hp.empty((T,))
    ws, wsb = hp.workspace(L.query("pdn_linear_ce_dx_deferred_workspace_bytes", T, V, K))
    L.call("pdn_linear_ce_dx_deferred_f32", logits._ptr, mx._ptr, parts, tg._ptr, 1.0 / T, w._ptr, dx._ptr, lse._ptr, T, V, K, ws, wsb,
           hp.stream())
    dw, db = hp.empty((K, V)), hp.empty((V,))
    need = L.query("pdn_linear_ce_workspace_bytes", T, V, K)
    extra = (T // 32) * 37888 + 1152
    assert T >= 32768 and V >= 128 and need > extra, "the split kernel does not take this shape"
    ws, _ = hp.workspace(need)

    def bench(fn, iters=6):
        for _ in range(2):
            fn()
        hp.synchronize()
        with hp.Timer() as t:
            for _ in range(iters):
                fn()
        return t.ms / iters * 1e3

    def entry(nbytes):
        return lambda: L.call("pdn_linear_ce_backward_f32", x._ptr, K, logits._ptr, lse._ptr, tg._ptr, 1.0 / T, None, w._ptr, None, None,
                              dw._ptr, 0.0, db._ptr, 0.0, T, V, K, ws, nbytes, hp.stream())

    fl = 2.0 * T * V * K
    rows = []
    if ab == "0":
        rows.append(("fp32 MFMA kernel", entry(need - extra)))
    rows.append(({"0": "split fp16", "1": "split fp16, constant planes (MFMA + LDS)",
                  "2": "split fp16, logits fetched once (no HBM stream)"}[ab], entry(need)))
    for name, fn in rows:
        us = bench(fn)
        print(f"{name:48s} {us:9.1f} us   {fl / us / 1e-6 / 1e12:7.1f} TFLOP/s (2 M V K)   "
              f"{4.0 * T * V / us / 1e-6 / 1e12:5.2f} TB/s of logits", flush=True)


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    V = int(sys.argv[2]) if len(sys.argv) > 2 else 32000
    for ab in ("0", "1", "2"):
        env = dict(os.environ, PDN_LMHEAD_DW_SPLIT_ABLATE=ab)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(T), str(V)], env=env, timeout=240).returncode
        if rc != 0:
            print(f"variant {ab} ended with status {rc}: nothing more is started", flush=True)
            sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
