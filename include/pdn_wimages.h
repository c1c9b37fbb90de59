/* All weight plane images of a training pass in one launch (csrc/weight_images.hip), exported by libpdnhip.so beside
 * include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams) are the
 * core header's.  A header and a prefix (pdnw_) of their own for the reason given in include/pdn_optim.h;
 * tests/test_wimages_abi_cpu.py holds header = exports.
 *
 * The split-fp16 products of a layer (q | k | v + RoPE, gate | up + SwiGLU, dh + SwiGLU backward, the down projection, the
 * 288 x 288 products and the layer input gradients) each turn their weight into fp16 plane images first, in one or two small
 * launches per call that sit in front of the product.  Nothing changes a weight inside a forward pass or inside a backward
 * pass, so a caller that knows the pass's products may have all their images built at once:
 *
 *   1. fill one descriptor record (pdnw_desc_bytes() bytes each, opaque) per (weight, form) with the constructor that takes
 *      the arguments of the product's own entry;
 *   2. pdnw_set_build builds every image of the set into an arena of pdnw_set_bytes bytes in ONE launch (one more per
 *      48 descriptors).  The images are byte for byte those of the per-call passes: both compile the same device code;
 *   3. pdnw_bind makes the set the calling thread's current one.  A product launched on the bound stream whose weight
 *      operand, form, leading dimension and block layout equal a record's takes that image and launches no pass of its own;
 *      any other product does exactly what it does with nothing bound;
 *   4. pdnw_unbind before the arena is released or a weight of the set is changed.
 *
 * The library keeps no image beyond that: the arena is the caller's, and a set describes the weights as they were when it
 * was built.  PDN_WIMAGES=0, read on every pdnw_bind and announced once, makes pdnw_bind do nothing.
 * Every entry returns PDN_EINVAL for arguments outside the product's own contract (contraction 288 for the first three,
 * 16-byte aligned operands, strides that are multiples of 4). */
#ifndef PDN_WIMAGES_H
#define PDN_WIMAGES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int64_t pdnw_desc_bytes(void);
/* the weight operands of pdn_qkv_rope_fwd_f32 (and its _norm forms): Wq | Wk | Wv, (K x D) each, w_stride floats apart */
int pdnw_desc_qkv(void* desc, const float* wq, int64_t w_stride, int D, int K);
/* of pdn_gateup_swiglu_fwd_f32 (and its _norm forms): Wg, Wu (K x F), w_stride floats apart (negative: up below gate) */
int pdnw_desc_gateup(void* desc, const float* w_gate, int64_t w_stride, int F, int K);
/* of pdn_swiglu_bwd_gemm_f32: W_down (F x K), read along K */
int pdnw_desc_down_t(void* desc, const float* w_down, int F, int K);
/* of the output-resident products C (M x 288) = A (M x K) B: b_trans 0: B (K x 288) row-major, ldb floats between rows
 * (pdn_gemm_f32 with N = 288: the down projection, ctx Wo); b_trans 1, kb 0: B = W^T, W (288 x K) with ldb floats between
 * rows (dz Wo^T); b_trans 1, kb > 0: W as K / kb blocks (288 x kb), b_bstride floats apart, ldb = kb
 * (pdn_gemm_outres_blocks_nt_f32, pdng_outres_blocks_nt_rmsnorm_bwd_f32) */
int pdnw_desc_outres(void* desc, const float* B, int K, int64_t ldb, int b_trans, int kb, int64_t b_bstride);

/* descs: n records, contiguous, in host memory.  arena: device memory, 256-byte aligned, at least pdnw_set_bytes bytes. */
int64_t pdnw_set_bytes(const void* descs, int n);
int pdnw_set_build(const void* descs, int n, void* arena, void* stream);
int pdnw_bind(const void* descs, int n, void* arena, void* stream);
int pdnw_unbind(void);
/* launches of pdnw_set_build, images products took from a bound set, and products that ran a pass of their own, so far in
 * this process (any of the pointers may be null); reset != 0 zeroes the three after reading */
int pdnw_stats(int64_t* builds, int64_t* hits, int64_t* passes, int reset);

#ifdef __cplusplus
}
#endif
#endif
