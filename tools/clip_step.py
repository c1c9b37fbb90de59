"""Times one CLIP ViT-B/32 training step (CLIP.finetune_step, every parameter trainable, Adam) on the MI355X.

N images (3 x 224 x 224) against K = N texts of 77 tokens, targets arange(N), random weights 0.02 * randn.  Prints
ms / step, image-text pairs / s, the model FLOPs of a step computed from the shapes (forward + backward; the image itself
gets no gradient) and their share of the 157.3 TFLOP/s fp32-MFMA peak, then the same for `fused.patch_embed.enabled`
False (the generic nodes of llm/clip/model.py:17-32, 129-130) as an A/B of the patch-embedding kernels.  Timed with
device events over `--steps` steps after `--warmup` steps.  Needs a GPU.

    python tools/clip_step.py --batch 256 [--steps 10] [--warmup 3] [--no-ab]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3          # MI355X fp32 MFMA (dense)


def model_flops(N, K, img=224, p=32, Dv=768, Fv=3072, Lv_layers=12, Dt=512, Ft=2048, Lt_layers=12, Lt=77, E=512):
    """Multiply-adds x 2 of the GEMMs and attention products of one step: forward F, backward 2 F minus the image
    gradient of the patch projection (not formed)."""
    P = (img // p) ** 2
    Tv, Kp = P + 1, 3 * p * p

    def block(T, D, F):                                       # q|k|v, o, fc1, fc2 + q k^T, p v
        return 2 * T * (4 * D * D + 2 * D * F) + 4 * T * T * D
    patch = 2 * P * Kp * Dv
    image = patch + Lv_layers * block(Tv, Dv, Fv) + 2 * Dv * E
    text = Lt_layers * block(Lt, Dt, Ft) + 2 * Dt * E
    fwd = N * image + K * text + 2 * N * K * E
    return fwd + 2 * fwd - N * patch, fwd / max(N, 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-ab", action="store_true", help="skip the patch_embed.enabled = False run")
    args = ap.parse_args()

    import pydynet_amd as pdn
    from pydynet_amd import cuda, hipnp as hp
    from pydynet_amd.core import fused
    from pydynet_amd.core.tensor import Graph
    from pydynet_amd.llm.clip import CLIP
    from pydynet_amd.optim import Adam
    if not cuda.is_available():
        sys.exit("clip_step.py: no GPU (this tool times the HIP kernels on an MI355X)")
    hp.set_device(0)

    N = K = args.batch
    rng = np.random.default_rng(0)
    np.random.seed(0)
    model = CLIP()
    for p in model._parameters.values():
        if p.requires_grad:
            p.data[...] = (0.02 * rng.standard_normal(p.shape)).astype(np.float32)
    model.to("hip:0")
    img = pdn.Tensor(rng.standard_normal((N, 3, 224, 224)).astype(np.float32), device="hip:0")
    idx = rng.integers(1, 49000, (K, 77)).astype(np.int64)
    idx[np.arange(K), rng.integers(5, 77, K)] = 49407            # one end-of-text token per text
    tgt = np.arange(N)
    opt = Adam(model.parameters(), lr=1e-5)
    flops, fwd_per_pair = model_flops(N, K)

    def run(label):
        for _ in range(args.warmup):
            Graph.clear()
            model.finetune_step(img, idx, tgt, opt)
        hp.synchronize()
        e0 = hp.Event().record()
        losses = []
        for _ in range(args.steps):
            Graph.clear()
            losses.append(model.finetune_step(img, idx, tgt, opt))
        e1 = hp.Event().record()
        ms = e0.elapsed_ms(e1) / args.steps
        tf = flops / (ms * 1e-3) / 1e12
        r = {"config": label, "batch": N, "texts": K, "ms_per_step": round(ms, 3), "pairs_per_s": round(N / (ms * 1e-3), 1),
             "gflop_per_step": round(flops / 1e9, 1), "gflop_per_pair_fwd_bwd": round(flops / N / 1e9, 2),
             "tflops": round(tf, 2), "fraction_of_fp32_mfma_peak": round(tf / PEAK_TFLOPS, 4),
             "loss_first": round(losses[0], 5), "loss_last": round(losses[-1], 5)}
        print(json.dumps(r), flush=True)
        return r

    fused_r = run("patch_embed kernels")
    if not args.no_ab:
        fused.patch_embed.enabled = False
        try:
            generic = run("patch_embed generic nodes")
        finally:
            fused.patch_embed.enabled = True
        print(json.dumps({"patch_embed_ab_ms_saved_per_step": round(generic["ms_per_step"] - fused_r["ms_per_step"], 3),
                          "speedup": round(generic["ms_per_step"] / fused_r["ms_per_step"], 4)}), flush=True)


if __name__ == "__main__":
    main()
