/* The block norms' outputs are never written (csrc/normplanes.hip, csrc/split_tn_planes.hip, csrc/gemm_rowres.hip), exported
 * by libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes,
 * pdn_last_error, streams) are the core header's.  A header and a prefix (pdnp_) of their own for the reason given in
 * include/pdn_optim.h; tests/test_normplanes_abi_cpu.py holds header = exports = emulation.
 *
 * With xn = rmsnorm(x) = x * (1 / rms) * norm_w over 288 columns, rms[t] = sqrt(mean_d x[t][d]^2 + eps):
 *
 *   forward   pdn_gateup_swiglu_norm_fwd_f32 and pdn_qkv_rope_norm_fwd_f32 WITHOUT their xn argument: the same launches,
 *             the same gu / h / qkv / rms, bit for bit; the normalised rows are not stored.  Served by the split-fp16
 *             projection kernel alone (16384 rows and more, PDN_ROWTILE_SPLIT not 0, no captured stream): ask *_supported,
 *             which reads the switches; elsewhere the entries fail with PDN_EUNSUPPORTED / PDN_EINVAL and launch nothing.
 *   backward  pdnp_norm_dw_blocks_f32: the packed weight gradients dW_b = beta dW_b + xn^T G_b, b = 0 .. nb - 1, from x,
 *             norm_w and rms.  Where the split-fp16 TN kernel takes the product (288 rows, nb >= 2 blocks of nb_cols columns,
 *             768 .. 8192 columns in all, K >= 32768 a multiple of 32, PDN_OUTRES_TN_SPLIT not 0, 16-byte alignment) its
 *             plane pass forms xn on the way into the fp16 planes in ONE launch and xn exists nowhere: the power of two of
 *             column d is that of the bound |xn[t][d]| < 17 |norm_w[d]| instead of the column's maximum (a zero or
 *             non-finite norm_w[d]: exponent 0).  Otherwise the entry writes xn into its workspace and runs pdn_gemm_f32
 *             on it.  PDN_NORM_PLANES=0, read on every call and announced once, forces that.  Deterministic either way.
 *
 * CONTRACT of the backward entry: rms[t] >= sqrt(mean_d x[t][d]^2), which is what the forward writes.  With a smaller rms
 * the bound does not hold, a plane may overflow to Inf and the column comes out NaN.  A non-finite row of x comes out NaN in
 * every dW entry it contributes to, as in pdn_gemm_f32. */
#ifndef PDN_NORMPLANES_H
#define PDN_NORMPLANES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int pdnp_gateup_swiglu_norm_supported(int M, int F, int K);
int pdnp_gateup_swiglu_norm_fwd_f32(const float* x, const float* norm_w, float eps, float* rms, const float* w_gate,
                                    int64_t w_stride, float* gu, float* h, int M, int F, int K, int64_t ldx, void* stream);
int pdnp_qkv_rope_norm_supported(int M, int D, int K, int L, int hd);
int pdnp_qkv_rope_norm_fwd_f32(const float* x, const float* norm_w, float eps, float* rms, const float* wq, int64_t w_stride,
                               float* qkv, const float* rope, int M, int D, int K, int L, int hd, int64_t ldx, void* stream);

/* x (K x 288) contiguous, norm_w (288), rms (K); G (K x nb * nb_cols, rows ldg floats apart); dW_b (288 x nb_cols) contiguous,
 * dw_block_stride floats apart.  workspace: at least pdnp_norm_dw_blocks_workspace_bytes(K, nb_cols, nb) bytes, 16-byte
 * aligned. */
int pdnp_norm_dw_blocks_f32(const float* x, const float* norm_w, const float* rms, const float* G, int64_t ldg, float* dW,
                            int64_t dw_block_stride, float beta, int K, int nb_cols, int nb, void* workspace,
                            int64_t workspace_bytes, void* stream);
/* the product's own workspace (pdn_gemm_f32_workspace_bytes, at most 256 MiB), and room for xn unless the plane route is to be
 * expected from (K, nb_cols, nb), PDN_NORM_PLANES and PDN_OUTRES_TN_SPLIT as they are read at the query.  Where xn is needed
 * all the same (operands off 16 bytes, a switch set since) the entry takes it from the library's allocator; in a captured
 * stream it returns PDN_EWORKSPACE and names the bytes it needs. */
int64_t pdnp_norm_dw_blocks_workspace_bytes(int K, int nb_cols, int nb);
/* whether the entry takes the shape at all: nb_cols a multiple of 4, any K */
int pdnp_norm_dw_blocks_supported(int K, int nb_cols, int nb);
/* calls so far that ran the one-launch plane pass (the other route counts nothing here); reset != 0 zeroes the count after
 * reading */
int64_t pdnp_norm_dw_blocks_plane_launches(int reset);

#ifdef __cplusplus
}
#endif
#endif
