"""The two halves of include/pdn_normplanes.h at 131072 rows, each against what it replaces, alternating in one process:

  * the packed weight gradient behind a block norm -- dW_q|k|v (3 x 288 columns) and dW_gate|up (2 x 768) -- as the existing
    route (pdn_gemm_f32 on the xn the forward wrote: three plane launches + product + slab reduce) against
    pdnp_norm_dw_blocks_f32 on (x, norm_w, rms) (one plane launch + the same product and reduce), and against that entry with
    PDN_NORM_PLANES=0 (xn written into the workspace first);
  * the two forward projections with the xn store (pdn_*_norm_fwd_f32) and without (pdnp_*_norm_fwd_f32).

`rounds` rounds of `calls` calls each; minimum, median and maximum over the rounds.  Before the timing the results are compared
once and the plane-launch counter is read.
usage: python tools/norm_planes_probe.py [rows=131072] [rounds=5] [calls=10]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, F, HD, SEQ = 288, 768, 48, 256


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    sys.path.insert(0, ROOT)
    import numpy as np
    from pydynet_amd import hipnp as hp, _lib
    hp.set_device(0)
    L = _lib.lib()
    rng = np.random.default_rng(0)

    def timed(fn):
        fn()
        hp.synchronize()
        with hp.Timer() as t:
            for _ in range(calls):
                fn()
        return t.ms / calls * 1e3

    def report(tag, us):
        for v, t in us.items():
            t = sorted(t)
            print(f"{tag}  {v:22s} {t[len(t) // 2]:8.1f} us (min {t[0]:7.1f}, max {t[-1]:7.1f})", flush=True)

    x = hp.from_numpy(rng.standard_normal((M, D), dtype=np.float32))
    w = hp.from_numpy((1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
    wq = hp.from_numpy(0.05 * rng.standard_normal((3, D, D), dtype=np.float32))
    wgu = hp.from_numpy(0.05 * rng.standard_normal((2, D, F), dtype=np.float32))
    ang = rng.uniform(0, 6.28, (SEQ, HD)).astype(np.float32)
    tab = hp.from_numpy(np.stack([np.cos(ang), -np.sin(ang)], -1).astype(np.float32))
    xn, rms, rms2 = hp.empty((M, D), np.float32), hp.empty((M,), np.float32), hp.empty((M,), np.float32)
    qkv, qkv2 = hp.empty((M, 3 * D), np.float32), hp.empty((M, 3 * D), np.float32)
    gu, gu2 = hp.empty((M, 2 * F), np.float32), hp.empty((M, 2 * F), np.float32)
    h, h2 = hp.empty((M, F), np.float32), hp.empty((M, F), np.float32)

    # ---- forward: with and without the xn store
    def qkv_old():
        L.call("pdn_qkv_rope_norm_fwd_f32", x._ptr, w._ptr, 1e-6, xn._ptr, rms._ptr, wq._ptr, D * D, qkv._ptr, tab._ptr, M, D, D, SEQ,
               HD, D, hp.stream())

    def qkv_new():
        L.call("pdnp_qkv_rope_norm_fwd_f32", x._ptr, w._ptr, 1e-6, rms2._ptr, wq._ptr, D * D, qkv2._ptr, tab._ptr, M, D, D, SEQ, HD, D,
               hp.stream())

    def gu_old():
        L.call("pdn_gateup_swiglu_norm_fwd_f32", x._ptr, w._ptr, 1e-6, xn._ptr, rms._ptr, wgu._ptr, D * F, gu._ptr, h._ptr, M, F, D, D,
               hp.stream())

    def gu_new():
        L.call("pdnp_gateup_swiglu_norm_fwd_f32", x._ptr, w._ptr, 1e-6, rms2._ptr, wgu._ptr, D * F, gu2._ptr, h2._ptr, M, F, D, D,
               hp.stream())

    assert L.query("pdnp_qkv_rope_norm_supported", M, D, D, SEQ, HD) and L.query("pdnp_gateup_swiglu_norm_supported", M, F, D)
    for name, old, new, pairs in (("q | k | v + RoPE", qkv_old, qkv_new, lambda: ((qkv, qkv2), (rms, rms2))),
                                  ("gate | up + SwiGLU", gu_old, gu_new, lambda: ((gu, gu2), (h, h2), (rms, rms2)))):
        old()
        new()
        hp.synchronize()
        same = all(np.array_equal(a.get().view(np.uint32), b.get().view(np.uint32)) for a, b in pairs())
        us = {"with xn": [], "without xn": []}
        for _ in range(rounds):
            us["with xn"].append(timed(old))
            us["without xn"].append(timed(new))
        tag = f"{M} rows {name:18s}"
        print(f"{tag}  outputs and rms bit-identical: {same}", flush=True)
        report(tag, us)
        print(f"{tag}  with min - without min = {min(us['with xn']) - min(us['without xn']):6.1f} us", flush=True)

    # ---- backward: the packed weight gradients (xn, rms: as the gate | up forward above left them)
    for name, nbc, nb in (("dW q | k | v", D, 3), ("dW gate | up", F, 2)):
        g = hp.from_numpy(1e-3 * rng.standard_normal((M, nb * nbc), dtype=np.float32))
        gb = hp.ndarray(g._buf, g._ptr, (nb, M, nbc), (nbc, nb * nbc, 1), g.dtype)
        dw_o, dw_n, dw_f = (hp.zeros((nb, D, nbc), np.float32) for _ in range(3))
        nbytes = L.query("pdnp_norm_dw_blocks_workspace_bytes", M, nbc, nb)
        os.environ["PDN_NORM_PLANES"] = "0"
        fbytes = L.query("pdnp_norm_dw_blocks_workspace_bytes", M, nbc, nb)
        os.environ.pop("PDN_NORM_PLANES", None)
        wsb = hp.empty((max(nbytes, fbytes),), np.bool_)

        def old():
            hp.gemm(xn.T, gb, dw_o)

        def entry(out=dw_n):
            L.call("pdnp_norm_dw_blocks_f32", x._ptr, w._ptr, rms._ptr, g._ptr, nb * nbc, out._ptr, D * nbc, 0.0, M, nbc, nb, wsb._ptr,
                   max(nbytes, fbytes), hp.stream())

        n0 = L.query("pdnp_norm_dw_blocks_plane_launches", 0)
        old()
        entry()
        n1 = L.query("pdnp_norm_dw_blocks_plane_launches", 0)
        os.environ["PDN_NORM_PLANES"] = "0"
        entry(dw_f)
        os.environ.pop("PDN_NORM_PLANES", None)
        hp.synchronize()
        o, n, f = dw_o.get(), dw_n.get(), dw_f.get()
        ref = (x.get().astype(np.float64) / rms.get().astype(np.float64)[:, None] * w.get().astype(np.float64)).T @ g.get()[:, :64].astype(np.float64)
        e_o = float(np.abs(o[0][:, :64] - ref).max() / np.abs(ref).max())
        e_n = float(np.abs(n[0][:, :64] - ref).max() / np.abs(ref).max())
        tag = f"{M} rows {name:18s}"
        print(f"{tag}  plane launches {n1 - n0}; error against float64 (64 columns): existing {e_o:.2e}, one launch {e_n:.2e}; "
              f"one launch vs existing {float(np.abs(n - o).max() / np.abs(o).max()):.2e}; switch off bit-identical to existing: "
              f"{np.array_equal(f.view(np.uint32), o.view(np.uint32))}", flush=True)
        us = {"three launches + product": [], "one launch + product": [], "entry, switch off": []}
        for _ in range(rounds):
            us["three launches + product"].append(timed(old))
            us["one launch + product"].append(timed(entry))
            os.environ["PDN_NORM_PLANES"] = "0"
            us["entry, switch off"].append(timed(lambda: entry(dw_f)))
            os.environ.pop("PDN_NORM_PLANES", None)
        report(tag, us)
        print(f"{tag}  three min - one min = {min(us['three launches + product']) - min(us['one launch + product']):6.1f} us", flush=True)


if __name__ == "__main__":
    main()
