"""The row-resident projections with a fused epilogue -- q | k | v + RoPE and gate | up + SwiGLU, each with and without
the RMSNorm folded in, and dh + SwiGLU backward -- timed in isolation on the fp32 MFMA kernel (`pdn_gemm_rowtile_mode(3)`, csrc/gemm_rowtile.hip) and on
split fp16 (csrc/rowtile_split.hip; the figure includes the W pass).  The library reads PDN_ROWTILE_SPLIT_ABLATE once: run the
probe again with it set to 1 (stores off) or 2 (constant planes: the rows of x are neither read nor normalised, xn is not
written) or 4 (dh + SwiGLU backward only: the gu rows are not read) to see where the time goes -- the results are then WRONG
and the library says so.  With rounds > 1 the two forms alternate `rounds` times and the smallest and largest time are printed.
usage: python tools/rowtile_split_probe.py [tokens=131072] [ffn=768] [seq=256] [head_dim=48] [rounds=1]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pydynet_amd import hipnp as hp, _lib

hp.set_device(0)
L = _lib.lib()
T = int(sys.argv[1]) if len(sys.argv) > 1 else 131072
F = int(sys.argv[2]) if len(sys.argv) > 2 else 768
Lq = int(sys.argv[3]) if len(sys.argv) > 3 else 256
hd = int(sys.argv[4]) if len(sys.argv) > 4 else 48
ROUNDS = int(sys.argv[5]) if len(sys.argv) > 5 else 1
K = D = 288
EPS = 1e-6
rng = np.random.default_rng(0)
x = hp.from_numpy(rng.standard_normal((T, K), dtype=np.float32))
wn = hp.from_numpy(rng.uniform(0.5, 1.5, K).astype(np.float32))
wqkv = hp.from_numpy((0.08 * rng.standard_normal((3, K, D))).astype(np.float32))
wgu = hp.from_numpy((0.08 * rng.standard_normal((2, K, F))).astype(np.float32))
inv = 1.0 / (10000 ** (np.arange(0, hd, 2)[: hd // 2] / hd))
fr = np.outer(np.arange(Lq), inv)
cd, sd = hp.from_numpy(np.cos(fr).astype(np.float32)), hp.from_numpy(np.sin(fr).astype(np.float32))
tab = hp.empty((Lq, hd, 2))
L.call("pdn_rope_table_f32", cd._ptr, sd._ptr, tab._ptr, Lq, hd, hp.stream())
wdn = hp.from_numpy((0.08 * rng.standard_normal((F, K))).astype(np.float32))
qkv, gu, h, xn, rms = hp.empty((T, 3 * D)), hp.empty((T, 2 * F)), hp.empty((T, F)), hp.empty((T, K)), hp.empty((T,))
dgu = hp.empty((T, 2 * F))


def bench(fn, iters=10):
    for _ in range(3):
        fn()
    hp.synchronize()
    with hp.Timer() as t:
        for _ in range(iters):
            fn()
    return t.ms / iters * 1e3


entries = [
    ("q|k|v + RoPE", lambda: L.call("pdn_qkv_rope_fwd_f32", x._ptr, wqkv._ptr, K * D, qkv._ptr, tab._ptr, T, D, K, Lq, hd, K, hp.stream()),
     2.0 * T * 3 * D * K, 4.0 * (T * K + 3 * T * D)),
    ("norm + q|k|v + RoPE", lambda: L.call("pdn_qkv_rope_norm_fwd_f32", x._ptr, wn._ptr, EPS, xn._ptr, rms._ptr, wqkv._ptr, K * D, qkv._ptr,
                                          tab._ptr, T, D, K, Lq, hd, K, hp.stream()), 2.0 * T * 3 * D * K, 4.0 * (2 * T * K + 3 * T * D)),
    ("gate|up + SwiGLU", lambda: L.call("pdn_gateup_swiglu_fwd_f32", x._ptr, wgu._ptr, K * F, gu._ptr, h._ptr, T, F, K, K, hp.stream()),
     2.0 * T * 2 * F * K, 4.0 * (T * K + 3 * T * F)),
    ("norm + gate|up + SwiGLU", lambda: L.call("pdn_gateup_swiglu_norm_fwd_f32", x._ptr, wn._ptr, EPS, xn._ptr, rms._ptr, wgu._ptr, K * F,
                                              gu._ptr, h._ptr, T, F, K, K, hp.stream()), 2.0 * T * 2 * F * K, 4.0 * (2 * T * K + 3 * T * F)),
    # (after the entries above: gu holds a real forward result)
    ("dh + SwiGLU backward", lambda: L.call("pdn_swiglu_bwd_gemm_f32", x._ptr, wdn._ptr, gu._ptr, dgu._ptr, T, F, K, K, hp.stream()),
     2.0 * T * F * K, 4.0 * (T * K + 4 * T * F)),
]
ab = os.environ.get("PDN_ROWTILE_SPLIT_ABLATE", "0")
tag = {"0": "", "1": " (NO stores)", "2": " (constant planes)", "4": " (gu NOT read)"}.get(ab, f" (ablate {ab})")
print(f"{T} rows, F {F}, L {Lq}, hd {hd}")
for name, fn, fl, by in entries:
    t32, t16 = [], []
    for _ in range(ROUNDS):
        prev = L.query("pdn_gemm_rowtile_mode", 3)
        t32.append(bench(fn))
        L.query("pdn_gemm_rowtile_mode", 1)
        t16.append(bench(fn))
        L.query("pdn_gemm_rowtile_mode", prev)
    us32, us16 = min(t32), min(t16)
    spread = f"   [min .. max over {ROUNDS} rounds: fp32 {min(t32):.1f} .. {max(t32):.1f}, split {min(t16):.1f} .. {max(t16):.1f}]" if ROUNDS > 1 else ""
    print(f"{name:26s} fp32 {us32:8.1f} us ({fl / us32 / 1e6:6.1f} TFLOP/s)   split fp16{tag} {us16:8.1f} us "
          f"({fl / us16 / 1e6:6.1f} TFLOP/s, {by / us16 / 1e6:5.2f} TB/s of its {by / 1e6:.0f} MB){spread}", flush=True)
