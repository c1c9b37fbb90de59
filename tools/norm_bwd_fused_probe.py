"""The layer input gradient followed by the RMSNorm backward of a block norm at 131072 rows -- dX over q | k | v (K = 864 as
three blocks) and over gate | up (K = 1536 as two blocks at falling addresses) -- as the two launches
(pdn_gemm_outres_blocks_nt_f32, pdn_rmsnorm_bwd_f32) against the one call with the norm's backward in the product's drain
(pdng_outres_blocks_nt_rmsnorm_bwd_f32, csrc/normgrad.hip), each with and without the held gradient (dx_residual) and the
weight gradient (dw).  PDN_NORM_BWD_FUSE is read by the library on every call, so the pair and the fused call alternate in
one process: `rounds` rounds of `calls` calls each, minimum, median and maximum over the rounds.  Before the timing the two
routes' results are compared once (largest difference over the pair's largest entry) and the fused-launch counter is read.
usage: python tools/norm_bwd_fused_probe.py [rows=131072] [rounds=5] [calls=10]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 288


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

    x = hp.from_numpy(rng.standard_normal((M, D), dtype=np.float32))
    w = hp.from_numpy((1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32))
    xh = x.get().astype(np.float64)
    rms = hp.from_numpy(np.sqrt((xh * xh).mean(-1) + 1e-6).astype(np.float32))
    del xh
    ex = hp.from_numpy(rng.standard_normal((M, D), dtype=np.float32))
    for name, K, nb in (("dX over q | k | v", 864, 3), ("dX over gate | up", 1536, 2)):
        kb = K // nb
        a = hp.from_numpy(1e-3 * rng.standard_normal((M, K), dtype=np.float32))
        wt = hp.from_numpy(0.05 * rng.standard_normal((nb, D, kb), dtype=np.float32))
        w0, stride = wt._ptr + 4 * (nb - 1) * D * kb * (nb == 2), D * kb * (-1 if nb == 2 else 1)
        dxn = hp.empty((M, D), np.float32)
        nws, nwsb = hp.workspace(L.query("pdn_rmsnorm_bwd_workspace_bytes", M, D))
        fbytes = L.query("pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes", M, kb, nb)
        fbuf = hp.empty((fbytes,), np.bool_)
        for with_ex in (False, True):
            for with_dw in (False, True):
                exp = ex._ptr if with_ex else None
                dx_p, dx_f = hp.empty((M, D), np.float32), hp.empty((M, D), np.float32)
                dw_p, dw_f = hp.zeros((D,), np.float32), hp.zeros((D,), np.float32)

                def pair():
                    L.call("pdn_gemm_outres_blocks_nt_f32", a._ptr, w0, stride, kb, nb, dxn._ptr, None, M, K, D, hp.stream())
                    L.call("pdn_rmsnorm_bwd_f32", x._ptr, w._ptr, rms._ptr, dxn._ptr, exp, dx_p._ptr,
                           dw_p._ptr if with_dw else None, 0, M, D, nws, nwsb, hp.stream())

                def entry():
                    L.call("pdng_outres_blocks_nt_rmsnorm_bwd_f32", a._ptr, w0, stride, kb, nb, x._ptr, w._ptr, rms._ptr, exp,
                           dx_f._ptr, dw_f._ptr if with_dw else None, 0, M, K, fbuf._ptr, fbytes, hp.stream())

                os.environ.pop("PDN_NORM_BWD_FUSE", None)
                n0 = L.query("pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches", 0)
                pair()
                entry()
                hp.synchronize()
                n1 = L.query("pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches", 0)
                p, f = dx_p.get(), dx_f.get()
                ddx = float(np.abs(p - f).max()) / float(np.abs(p).max())
                ddw = float(np.abs(dw_p.get() - dw_f.get()).max()) / max(float(np.abs(dw_p.get()).max()), 1e-30) if with_dw else 0.0
                del p, f
                us = {"pair": [], "fused": [], "entry, switch off": []}
                for _ in range(rounds):
                    us["pair"].append(timed(pair))
                    us["fused"].append(timed(entry))
                    os.environ["PDN_NORM_BWD_FUSE"] = "0"
                    us["entry, switch off"].append(timed(entry))
                    os.environ.pop("PDN_NORM_BWD_FUSE", None)
                tag = f"{M} x {K:4d} {name:18s} ex={int(with_ex)} dw={int(with_dw)}"
                print(f"{tag}  fused launches {n1 - n0}  fused vs pair: dx {ddx:.2e} dw {ddw:.2e}", flush=True)
                for v, t in us.items():
                    t = sorted(t)
                    print(f"{tag}  {v:18s} {t[len(t) // 2]:8.1f} us (min {t[0]:7.1f}, max {t[-1]:7.1f})", flush=True)
                print(f"{tag}  pair min - fused min = {min(us['pair']) - min(us['fused']):6.1f} us", flush=True)


if __name__ == "__main__":
    main()
