/* The RMSNorm backward folded into the layer input gradient (csrc/normgrad.hip, csrc/outres_split.hip), exported by
 * libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes,
 * pdn_last_error, streams) are the core header's.  A header and a prefix (pdng_) of their own for the reason given in
 * include/pdn_optim.h; tests/test_normgrad_abi_cpu.py holds header = exports = emulation (tests/abi_emulator/_normgrad.py).
 *
 * Statement: pdn_gemm_outres_blocks_nt_f32 with no residual,
 *     d(xn) (M x 288) = [d_1 | ... | d_nb] (M x nb * kb, row stride lda) [W_1 | ... | W_nb]^T,
 * followed by pdn_rmsnorm_bwd_f32 on its output with 288 columns,
 *     z = x / rms,  dz = d(xn) w,  dx = (dz - z mean(z dz)) / rms + dx_residual,  dw (+)= sum over rows of d(xn) z.
 * x, dx_residual and dx are M x 288 and contiguous.  Where the split-fp16 output-resident kernel takes the product (65536
 * rows and more, no captured stream, PDN_OUTRES_SPLIT not 0, 16-byte alignment) the norm's backward runs in that kernel's
 * drain and d(xn) never exists; otherwise the entry runs the two launches of the statement itself, with d(xn) in the
 * workspace.  PDN_NORM_BWD_FUSE=0, read on every call and announced once, forces the two launches.  Deterministic either
 * way (no atomics). */
#ifndef PDN_NORMGRAD_H
#define PDN_NORMGRAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* dx_residual and dw may be NULL; accumulate_dw selects dw += over dw =.  workspace: at least
 * pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes(M, kb, nb) bytes, 16-byte aligned. */
int pdng_outres_blocks_nt_rmsnorm_bwd_f32(const float* A, const float* W, int64_t b_block_stride, int kb, int nb,
                                          const float* x, const float* w, const float* rms, const float* dx_residual,
                                          float* dx, float* dw, int accumulate_dw, int M, int64_t lda, void* workspace,
                                          int64_t workspace_bytes, void* stream);
/* the partial rows of dw, and room for d(xn) unless the fused route is to be expected from (M, kb, nb), PDN_NORM_BWD_FUSE and
 * PDN_OUTRES_SPLIT as they are read at the query.  Where the two launches run all the same (operands off 16 bytes, a switch
 * set since) the entry takes d(xn) from the library's allocator; in a captured stream it returns PDN_EWORKSPACE and names
 * the bytes it needs. */
int64_t pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes(int M, int kb, int nb);
/* whether the entry takes the shape at all: kb a multiple of 32, any row count (below the split kernel's 65536 rows the two
 * launches run whatever pdn_gemm_outres_blocks_supported says about their speed) */
int pdng_outres_blocks_nt_rmsnorm_bwd_supported(int M, int kb, int nb);
/* calls so far that ran the fused kernel (the other route counts nothing here); reset != 0 zeroes the count after reading */
int64_t pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches(int reset);

#ifdef __cplusplus
}
#endif
#endif
