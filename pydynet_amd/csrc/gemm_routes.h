// The functions of the other GEMM files that csrc/gemm.hip routes to (pdn_gemm_f32, pdn_linear_ce_backward_f32,
// pdn_linear_ce_dx_deferred_f32).  csrc/gemm.hip and the files that define them include this header, so the compiler checks
// every definition against the one declaration.  (The split-fp16 TN kernels are declared the same way in split_tn.h.)
#pragma once
#include <stdint.h>

// ---- csrc/gemm_narrow.hip: products with at most 16 output columns (bandwidth kernels)
bool pdn_gemm_narrow_nn_ok(int M, int N, int K, int64_t a_rs, int64_t a_cs, const void* A);
int pdn_gemm_narrow_nn_launch(const float* A, int64_t lda, const float* B, int64_t b_rs, int64_t b_cs, const float* bias,
                              float* C, int64_t ldc, int M, int N, int K, void* stream);
int pdn_gemm_narrow_tn_plan(int Mc, int N, int K, int64_t a_rs, int64_t a_cs, int64_t b_cs, const void* A, int64_t ws_cap_floats,
                            int* kps);
int pdn_gemm_narrow_tn_launch(const float* A, int64_t a_cs, const float* B, int64_t b_rs, float* slabs, int Mc, int N, int K,
                              int kps, int splits, void* stream);

// ---- csrc/gemm_outres.hip: the output-resident kernel (N = 288) and its weight-gradient (TN) form
extern "C" int64_t pdn_gemm_outres_workspace_bytes(int M, int K);
extern "C" int pdn_gemm_outres_plan(int M, int K, int* nw, int* kps);
extern "C" int pdn_gemm_outres_supported(int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int b_trans);
extern "C" int pdn_gemm_outres_f32(const float* A, const float* B, float* C, const float* bias,
                                   const float* residual, int M, int N, int K, int64_t lda, int64_t ldb,
                                   int64_t ldc, int b_trans, void* stream);
extern "C" int pdn_gemm_outres_ws_f32(const float* A, const float* B, float* C, const float* bias, const float* residual,
                                      int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int b_trans,
                                      void* workspace, int64_t workspace_bytes, void* stream);
int pdn_outres_blocks_nt_launch(const float* A, const float* W, int64_t b_block_stride, int kb, int nb, float* C, int M,
                                int64_t lda, int64_t ldc, void* stream);
int pdn_gemm_outres_tn_plan(int N, int K, int* nw_out, int* k_per_split_out);
int pdn_gemm_outres_tn_launch(const float* X, const float* G, float* C, int N, int K, int64_t ldx, int64_t ldg,
                              int64_t ldc, int64_t slab, int nw, int k_per_split, void* stream);
int pdn_gemm_outres_tn_blocks_launch(const float* X, const float* G, float* C, int N, int K, int64_t ldx, int64_t ldg,
                                     int nb_cols, int nw, int k_per_split, void* stream);
// ... with the gradient of `linear -> cross entropy` formed inside (pdn_linear_ce_backward_f32,
// pdn_linear_ce_dx_deferred_f32; the weight gradient on split-fp16 MFMA, csrc/lm_head_dw_split.hip: pdn_outres_ce_dw_split_*
// of split_tn.h)
int pdn_outres_ce_dx_launch(const float* logits, int64_t ldl, const float* lse, const int64_t* targets, float gscale,
                            const float* gdev, const float* W, int64_t ldw, float* dx, int64_t ldc,
                            const float* residual, int M, int V, void* workspace, int64_t workspace_bytes, void* stream);
int pdn_outres_ce_dw_launch(const float* X, const float* logits, float* C, int N, int K, int64_t ldx, int64_t ldg,
                            int64_t ldc, int64_t slab, int nw, int k_per_split, const float* lse,
                            const int64_t* targets, float gscale, const float* gdev, float* colsum, void* stream);
int pdn_outres_ce_dx_deferred_launch(const float* logits, int64_t ldl, const float* rowmax, int max_parts,
                                     const int64_t* targets, float gscale, const float* W, int64_t ldw, float* dx,
                                     int64_t ldc, float* lse_out, int M, int V, void* workspace, int64_t workspace_bytes,
                                     void* stream);
extern "C" int pdn_linear_ce_dx_deferred_supported(int64_t M, int V, int K);

// ---- csrc/outres_split.hip: the output-resident product on split-fp16 MFMA (65536 rows and more, K in [256, 4096], no K
// split); from pdn_gemm_f32 for the 288 x 288 products (slot 47)
int pdn_outres_split_takes(const float* A, const float* B, const float* C, const float* bias, const float* residual, int M,
                           int K, int64_t lda, int64_t ldb, int64_t ldc, int b_trans, int kb, int64_t b_bstride, int splits,
                           void* stream);
int pdn_outres_split_launch(const float* A, const float* B, float* C, const float* bias, const float* residual, int M, int K,
                            int64_t lda, int64_t ldb, int64_t ldc, int b_trans, int kb, int64_t b_bstride, void* stream,
                            int count_slot);
// ... with the RMSNorm backward of the product formed in the drain (csrc/normgrad.hip, include/pdn_normgrad.h)
int pdn_outres_split_norm_bwd_partial_rows(int M);
int pdn_outres_split_norm_bwd_launch(const float* A, const float* W, int64_t b_bstride, int kb, int nb, const float* x,
                                     const float* w, const float* rms, const float* ex, float* dx, float* dwpart, int M,
                                     int64_t lda, void* stream);

// ---- csrc/fused.hip: out[c] (+)= sum_b part[b][c] in a fixed order
int pdn_colsum_partials_launch(const float* part, int nb, int cols, float* out, int accumulate, void* stream);

// ---- csrc/gemm_rowres.hip: the row-resident / tile-piece kernels (K = 288)
extern "C" int pdn_gemm_rowres_supported(int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int b_trans);
int pdn_rowtile_plain_ok(int M, int N, int b_trans);
extern "C" int pdn_gemm_rowres_f32(const float* A, const float* B, float* C, const float* bias,
                                   const float* residual, int M, int N, int K, int64_t lda, int64_t ldb,
                                   int64_t ldc, int b_trans, void* stream);
int pdn_gemm_rowres_blocks(const float* A, const float* B, float* C, int M, int N, int K, int64_t lda, int64_t ldb,
                           int64_t ldc, int b_trans, int nblocks, int64_t b_block_stride, void* stream);
// ---- csrc/gemm_rowtile.hip
extern "C" int pdn_gemm_rowtile_mode(int mode);                 // a negative mode only asks

// ---- csrc/gemm.hip: route 7 (the packed layer weight gradients) with the A operand given as the rows before an RMSNorm, its
// weight and its row statistics, for csrc/normplanes.hip.  PDN_NORMPLANES_NOT_TAKEN: the split-fp16 form does not take the
// call (shape, switch, workspace, alignment) and nothing was launched.
#define PDN_NORMPLANES_NOT_TAKEN (-0x7fffffff)
int pdn_gemm_outres_tn_blocks_norm(const float* x, const float* norm_w, const float* rms, const float* G, int64_t ldg, float* dW,
                                   int64_t ldc, int64_t c_bs, float beta, int K, int nb_cols, int nb, void* workspace,
                                   int64_t workspace_bytes, void* stream);
