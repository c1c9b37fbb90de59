"""The output-resident products of a training step at 131072 rows -- dX = [dq | dk | dv] [Wq | Wk | Wv]^T (K = 864 as three
blocks), [dgate | dup] [Wg | Wu]^T (K = 1536 as two blocks at falling addresses) and the down projection h W_down + residual
(NN, K = 768) -- on the fp32 MFMA kernel (csrc/gemm_outres.hip) against the split-fp16 kernel (csrc/outres_split.hip: the
two W passes and the persistent product), the split kernel with one workgroup per 128-row block instead of 256 persistent
ones (PDN_OUTRES_SPLIT_WGS=0), and its timing ablations (PDN_OUTRES_SPLIT_ABLATE: 1 = constant planes, A never read --
MFMA + LDS only; 2 = A fetched once -- no HBM stream in; 3 = nothing stored).  The library reads these switches on every
call, so all variants alternate in one process, `rounds` times; the table shows the median of each.
Behind them the 288 x 288 products (K = 288, nine pieces: ctx Wo + x, NN with residual, and dz Wo^T, NT) through hipnp.gemm:
the fp32 tile-piece kernel (pdn_gemm_rowtile_mode(3)) against the same split kernel and its variants (counter slot 47).
usage: python tools/outres_split_probe.py [rows=131072] [rounds=5]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 288
VARIANTS = [("fp32 MFMA kernel", {"PDN_OUTRES_SPLIT": "0"}),
            ("split fp16, 256 persistent workgroups", {}),
            ("split fp16, one workgroup per block", {"PDN_OUTRES_SPLIT_WGS": "0"}),
            ("split, constant planes (MFMA + LDS)", {"PDN_OUTRES_SPLIT_ABLATE": "1"}),
            ("split, A fetched once (no stream in)", {"PDN_OUTRES_SPLIT_ABLATE": "2"}),
            ("split, nothing stored", {"PDN_OUTRES_SPLIT_ABLATE": "3"})]
SWITCHES = ("PDN_OUTRES_SPLIT", "PDN_OUTRES_SPLIT_WGS", "PDN_OUTRES_SPLIT_ABLATE")


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sys.path.insert(0, ROOT)
    import numpy as np
    from pydynet_amd import hipnp as hp, _lib
    hp.set_device(0)
    L = _lib.lib()
    rng = np.random.default_rng(0)

    def timed(fn, iters=6):
        fn()
        hp.synchronize()
        with hp.Timer() as t:
            for _ in range(iters):
                fn()
        return t.ms / iters * 1e3

    for name, K, nb, nn in (("dX over q | k | v", 864, 3, False), ("dX over gate | up", 1536, 2, False), ("down projection", 768, 1, True)):
        a = hp.from_numpy(1e-3 * rng.standard_normal((M, K), dtype=np.float32))
        res = hp.from_numpy(rng.standard_normal((M, D), dtype=np.float32))
        c = hp.empty((M, D), np.float32)
        kb = K // nb
        if nn:
            w = hp.from_numpy(0.05 * rng.standard_normal((K, D), dtype=np.float32))
            fn = lambda: L.call("pdn_gemm_outres_f32", a._ptr, w._ptr, c._ptr, None, res._ptr, M, D, K, K, D, D, 0, hp.stream())
        else:
            w = hp.from_numpy(0.05 * rng.standard_normal((nb, D, kb), dtype=np.float32))
            w0, stride = w._ptr + 4 * (nb - 1) * D * kb * (nb == 2), D * kb * (-1 if nb == 2 else 1)
            fn = lambda: L.call("pdn_gemm_outres_blocks_nt_f32", a._ptr, w0, stride, kb, nb, c._ptr, res._ptr, M, K, D, hp.stream())
        us = {v: [] for v, _ in VARIANTS}
        for _ in range(rounds):
            for v, env in VARIANTS:
                for s in SWITCHES:
                    os.environ.pop(s, None)
                os.environ.update(env)
                us[v].append(timed(fn))
        for s in SWITCHES:
            os.environ.pop(s, None)
        fl, by = 2.0 * M * D * K, 4.0 * M * (K + 2 * D)
        for v, _ in VARIANTS:
            t = sorted(us[v])
            m = t[len(t) // 2]
            print(f"{M} x {K:4d} {name:18s} {v:40s} {m:8.1f} us (min {t[0]:7.1f}, max {t[-1]:7.1f})  {fl / m / 1e6:6.1f} TFLOP/s"
                  f"  {by / m / 1e6:5.2f} TB/s of A + C + residual", flush=True)

    # ---- the 288 x 288 products through pdn_gemm_f32 (hipnp.gemm): the attention output projection ctx Wo + x (NN,
    # residual) and its input gradient dz Wo^T (NT).  pdn_gemm_rowtile_mode(3) keeps the fp32 tile-piece kernel
    # gemm_rowtile_kernel<.., 6 / 0>; the default sends them to the split kernel above (nine pieces). ------------------------
    K = D
    a = hp.from_numpy(1e-3 * rng.standard_normal((M, K), dtype=np.float32))
    res = hp.from_numpy(rng.standard_normal((M, D), dtype=np.float32))
    c = hp.empty((M, D), np.float32)
    w = hp.from_numpy(0.05 * rng.standard_normal((K, D), dtype=np.float32))
    variants = [("fp32 tile-piece kernel (mode 3)", 3, {})] + [(v, 1, env) for v, env in VARIANTS[1:]]
    for name, fn, nbytes in (("ctx Wo + x (NN)", lambda: hp.gemm(a, w, c, residual=res), 4.0 * M * 3 * D),
                             ("dz Wo^T (NT)", lambda: hp.gemm(a, w.T, c), 4.0 * M * 2 * D)):
        us = {v: [] for v, _, _ in variants}
        for _ in range(rounds):
            for v, mode, env in variants:
                for s in SWITCHES:
                    os.environ.pop(s, None)
                os.environ.update(env)
                prev = L.query("pdn_gemm_rowtile_mode", mode)
                us[v].append(timed(fn))
                L.query("pdn_gemm_rowtile_mode", prev)
        for s in SWITCHES:
            os.environ.pop(s, None)
        fl = 2.0 * M * D * K
        for v, _, _ in variants:
            t = sorted(us[v])
            m = t[len(t) // 2]
            print(f"{M} x {K:4d} {name:18s} {v:40s} {m:8.1f} us (min {t[0]:7.1f}, max {t[-1]:7.1f})  {fl / m / 1e6:6.1f} TFLOP/s"
                  f"  {nbytes / m / 1e6:5.2f} TB/s of A + C (+ residual)", flush=True)


if __name__ == "__main__":
    main()
