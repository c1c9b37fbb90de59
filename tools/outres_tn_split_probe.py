"""The packed layer weight gradients -- x^T (288 x K) against dq | dk | dv (K x 864 as three blocks) and dgate | dup
(K x 1536 as two) -- on the fp32 MFMA kernel (csrc/gemm_outres.hip, gemm_outres_tn_kernel behind
pdn_gemm_outres_tn_blocks_launch) against the split-fp16 kernel (csrc/outres_tn_split.hip: the three passes over x of
csrc/split_tn_planes.hip and the product), and the split kernel's timing ablations (PDN_OUTRES_TN_SPLIT_ABLATE: 1 = constant planes, g never read -- MFMA +
LDS only; 2 = g fetched once -- no HBM stream, the split arithmetic stays).  Every figure is one call of pdn_gemm_f32 in the
batched form of the backward pass with beta = 1 and includes the slab reduction, which both kernels share; the fp32 kernel
is selected by the workspace size (include/pdn_hip.h).  The library reads the ablation switch once, so every variant runs
in a child process of its own, one after the other; a child that fails ends the probe.
usage: python tools/outres_tn_split_probe.py [tokens=131072]

`--down [tokens]`: the down-projection weight gradient dW_down (768 x 288) = h^T g2 of pdn_gemm_f32, beta = 1, passes and
slab reduction included: the split-fp16 form with the transposed store (the full workspace) against the wave-streaming fp32
kernel (the 64 slabs only), both alternating in one process, median of 5 rounds of 6 calls."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 288
SHAPES = [(3, 288), (2, 768)]


def child(T):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pydynet_amd import hipnp as hp, _lib
    hp.set_device(0)
    L = _lib.lib()
    ab = os.environ.get("PDN_OUTRES_TN_SPLIT_ABLATE", "0")
    rng = np.random.default_rng(0)
    x = hp.from_numpy(rng.standard_normal((T, D), dtype=np.float32))

    def bench(fn, iters=6):
        for _ in range(2):
            fn()
        hp.synchronize()
        with hp.Timer() as t:
            for _ in range(iters):
                fn()
        return t.ms / iters * 1e3

    for nb, N in SHAPES:
        n_all = nb * N
        g = hp.from_numpy((1e-3 * rng.standard_normal((T, n_all), dtype=np.float32)))
        c = hp.from_numpy(np.zeros((nb, D, N), np.float32))
        need = L.query("pdn_gemm_f32_workspace_bytes", D, N, T, nb)
        slabs, extra = 64 * D * n_all * 4, (T // 32) * 36864 + 1152
        assert need == slabs + extra, "the split kernel does not take this shape"
        ws, _ = hp.workspace(need)

        def entry(nbytes):
            return lambda: L.call("pdn_gemm_f32", D, N, T, 1.0, x._ptr, 1, D, g._ptr, n_all, 1, 1.0, c._ptr, N, None, 1, nb,
                                  0, 0, 0, N, 0, D * N, None, None, 0, ws, nbytes, hp.stream())

        fl = 2.0 * D * n_all * T
        rows = []
        if ab == "0":
            rows.append(("fp32 MFMA kernel", entry(slabs)))
        rows.append(({"0": "split fp16", "1": "split fp16, constant planes (MFMA + LDS)",
                      "2": "split fp16, g fetched once (no HBM stream)"}[ab], entry(need)))
        for name, fn in rows:
            us = bench(fn)
            print(f"{T} x {nb} x {N}  {name:44s} {us:9.1f} us   {fl / us / 1e-6 / 1e12:7.1f} TFLOP/s (2 288 N K)   "
                  f"{4.0 * T * n_all / us / 1e-6 / 1e12:5.2f} TB/s of g", flush=True)


def down(T):
    sys.path.insert(0, ROOT)
    import numpy as np
    from pydynet_amd import hipnp as hp, _lib
    hp.set_device(0)
    L = _lib.lib()
    rng = np.random.default_rng(0)
    M = 768
    a, b = rng.standard_normal((T, M), dtype=np.float32), rng.standard_normal((T, M), dtype=np.float32)
    h = hp.from_numpy(a / (1.0 + np.exp(-a)) * b)
    g2 = hp.from_numpy(1e-3 * rng.standard_normal((T, D), dtype=np.float32))
    c = hp.from_numpy(np.zeros((M, D), np.float32))
    need = L.query("pdn_gemm_f32_workspace_bytes", M, D, T, 1)
    slabs = 64 * M * D * 4
    assert need == slabs + (T // 32) * 36864 + 1152, "the split kernel does not take this shape"
    ws, _ = hp.workspace(need)

    def entry(nbytes):
        return lambda: L.call("pdn_gemm_f32", M, D, T, 1.0, h._ptr, 1, M, g2._ptr, D, 1, 1.0, c._ptr, D, None, 1, 1,
                              0, 0, 0, 0, 0, 0, None, None, 0, ws, nbytes, hp.stream())

    variants = [("fp32 wave-streaming kernel", entry(slabs)), ("split fp16, transposed store", entry(need))]
    times = {name: [] for name, _ in variants}
    for name, fn in variants:
        fn()
    hp.synchronize()
    for _ in range(5):
        for name, fn in variants:
            fn()
            hp.synchronize()
            with hp.Timer() as t:
                for _ in range(6):
                    fn()
            times[name].append(t.ms / 6 * 1e3)
    fl = 2.0 * M * D * T
    for name, _ in variants:
        v = sorted(times[name])
        print(f"{T} x {M} x {D} dW_down  {name:32s} {v[2]:9.1f} us (min {v[0]:7.1f}, max {v[4]:7.1f})   "
              f"{fl / v[2] / 1e-6 / 1e12:7.1f} TFLOP/s", flush=True)


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    for ab in ("0", "1", "2"):
        env = dict(os.environ, PDN_OUTRES_TN_SPLIT_ABLATE=ab)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(T)], env=env, timeout=240).returncode
        if rc != 0:
            print(f"variant {ab} ended with status {rc}: nothing more is started", flush=True)
            sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--down":
        down(int(sys.argv[2]) if len(sys.argv) > 2 else 131072)
    else:
        main()
