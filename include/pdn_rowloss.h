/* Cross entropy with reduction='none': extensions of the pdnhip C ABI (csrc/row_loss.hip), exported by libpdnhip.so beside
 * include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams, the
 * error flag) are the core header's.
 *
 * Why a header and a prefix (pdnr_) of their own: as for include/pdn_optim.h, include/pdn_loss.h and include/pdn_segattn.h --
 * the tests hold include/pdn_hip.h, the library's pdn_* exports and the closed registry of the host emulation equal.  This
 * header is listed in _lib.ROWLOSS_HEADER_PATHS and held to the same three-way equality by tests/test_rowloss_abi_cpu.py:
 * the library's pdnr_* exports, and the emulation in tests/abi_emulator/_rowloss.py with its own NOT_EMULATED.
 *
 * Every entry below extends the cross entropy of nn/functional.py:364-381; the reference always reduces to a scalar, so
 * there is no counterpart.  Statement: pydynet_amd/core/fused/row_loss.py.
 *
 *   valid[n] = !masked || targets[n] != ignore_index
 *   row[n]   = valid[n] ? lse[n] - logits[n][targets[n]] : 0                      the node's value, (rows,)
 *   u        = the upstream gradient, (rows,) floats on the device
 *   dlogits[n] = valid[n] ? (softmax(logits[n]) - onehot(targets[n])) * u[n] : exactly 0, whatever u[n] holds
 *
 * No count and no factor.  Nothing is read back by the host, every sum is formed in a fixed order without atomics, nothing
 * is allocated inside a call: a step built on these entries replays from a hipGraph over changing targets and weights.
 * Each entry counts once in launch counter slot 44. */
#ifndef PDN_ROWLOSS_H
#define PDN_ROWLOSS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the unfused node (nn/functional.py:364-381, no counterpart).  Its forward is pdn_cross_entropy_fwd_f32 /
 * pdnl_cross_entropy_fwd_f32, which leave loss_row and lse_row.  dlogits from the saved lse_row and the upstream vector u;
 * an ignored row is zero-filled by a select.  Rows of 4096 <= V <= 32768 floats with V % 4 == 0 and aligned rows pass
 * through registers, a 1024-thread workgroup per row, others are streamed; both walk on past the grid.  masked == 0: every
 * row is valid and a negative target wraps as in pdn_cross_entropy_bwd_f32. */
int pdnr_cross_entropy_bwd_rows_f32(const float* logits, const int64_t* targets, int masked, int64_t ignore_index,
                                    const float* lse_row, const float* u, float* dlogits, int64_t rows, int V, void* stream);

/* ---- the lm_head + loss node (nn/functional.py:364-381 behind llm/llama/model.py:179, no counterpart).
 * The finish after the projection, pdnl_linear_ce_finish_f32 without the reduction: loss_row[n] as above,
 * targets_safe[n] = targets[n], or V for an ignored row (0, and *err_flag raised, for a valid one outside [0, V)), and
 * lse[n] = +inf for an ignored row, written IN PLACE. */
int pdnr_linear_ce_finish_rows_f32(const float* logits, int64_t ldl, float* lse, const int64_t* targets, int masked,
                                   int64_t ignore_index, int64_t rows, int V, float* loss_row, int64_t* targets_safe,
                                   int* err_flag, void* stream);
/* out[n][:] = targets_safe[n] != V ? in[n][:] * u[n] * inv_s[0] : 0 (inv_s NULL: 1); out may be in.  float4 where
 * cols, both leading dimensions and both addresses allow it (nn/functional.py:364-381, no counterpart). */
int pdnr_scale_rows_f32(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows, int cols, const float* u,
                        const float* inv_s, const int64_t* targets_safe, int V, void* stream);
/* s_out[0] = s = max |u[n]| over rows with targets_safe[n] != V, s_out[1] = s > 0 ? 1 / s : 0; one workgroup
 * (nn/functional.py:364-381, no counterpart). */
int pdnr_abs_max_rows_f32(const float* u, const int64_t* targets_safe, int V, int64_t rows, float* s_out, void* stream);
/* bytes of workspace of pdnr_weighted_colsum_f32 (nn/functional.py:364-381, no counterpart) */
int64_t pdnr_weighted_colsum_workspace_bytes(int64_t rows, int V);
/* dbias[v] = db_beta * dbias[v] + sum_n u[n] * (exp(logits[n][v] - lse[n]) - [v == targets_safe[n]]) over the rows with
 * targets_safe[n] != V: one pass over the saved logits, workgroups own row slabs x column ranges and leave partial rows in
 * the workspace, a second launch adds them in their order (nn/functional.py:364-381, no counterpart). */
int pdnr_weighted_colsum_f32(const float* logits, int64_t ldl, const float* lse_masked, const int64_t* targets_safe,
                             const float* u, int64_t rows, int V, float* dbias, float db_beta, void* workspace,
                             int64_t workspace_bytes, void* stream);
/* The backward of the node around the unchanged pdn_linear_ce_backward_f32, under its shape rules, alignment and workspace
 * size (pdn_linear_ce_workspace_bytes; the split-fp16 weight gradient is taken when the workspace holds its region).
 * lse_masked / targets_safe: what pdnr_linear_ce_finish_rows_f32 left.
 * dx (rows x in_features, may be NULL): the product with gscale 1 and no upstream, then its rows scaled by u.
 * dx_deferred (may be NULL, exclusive with dx): the product the forward pass left with gscale 1, scaled in place.
 * Either way rows of ignored tokens are exactly 0.
 * dW (may be NULL): x^T diag(u) dz = (diag(u / s) x)^T (s dz), s = max |u| over kept rows: xs (rows x in_features floats,
 * 16-byte aligned scratch, needed with dW) receives diag(u / s) x, s_out (2 floats, needed with dW) receives {s, 1 / s} and
 * the product reads s as its upstream device scalar.  s == 0 leaves dW = dw_beta * dW.
 * dbias (may be NULL): pdnr_weighted_colsum_f32 with colsum_workspace -- the product's own column sums are unweighted.
 * The column sums are launched before the products, so colsum_workspace may be the same memory as workspace.
 * (nn/functional.py:364-381, no counterpart) */
int pdnr_linear_ce_backward_rows_f32(const float* x, int64_t ldx, const float* logits, const float* lse_masked,
                                     const int64_t* targets_safe, const float* u, const float* W, float* dx,
                                     float* dx_deferred, float* dW, float dw_beta, float* dbias, float db_beta, float* xs,
                                     float* s_out, int64_t rows, int V, int in_features, void* workspace,
                                     int64_t workspace_bytes, void* colsum_workspace, int64_t colsum_workspace_bytes,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
