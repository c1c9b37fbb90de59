/* Cross entropy with ignore_index: extensions of the pdnhip C ABI (csrc/masked_loss.hip), exported by libpdnhip.so beside
 * include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams, the
 * error flag) are the core header's.
 *
 * Why a header and a prefix (pdnl_) of their own: as for include/pdn_optim.h -- the tests hold include/pdn_hip.h, the library's
 * pdn_* exports and the closed registry of the host emulation equal, and tests/test_optim_abi_cpu.py does the same for the
 * pdnx_* entries and _lib.EXT_HEADER_PATHS.  This header is listed in _lib.LOSS_HEADER_PATHS and held to the same three-way
 * equality by tests/test_loss_abi_cpu.py: the library's pdnl_* exports, and the emulation in tests/abi_emulator/_loss.py with
 * its own NOT_EMULATED.
 *
 * Every entry below extends the cross entropy of nn/functional.py:364-381; the reference has no ignore_index, so there is
 * no counterpart.  Statement: pydynet_amd/core/fused/masked_loss.py.
 *
 *   valid[n] = targets[n] != ignore_index        (any int64, an id inside [0, V) included)
 *   count = sum(valid);  factor = mean ? (count ? 1 / count : 0) : 1
 *   loss = factor * sum over valid rows of (lse[n] - logits[n][targets[n]]);    no valid row: loss 0, every gradient 0
 *   dlogits[n] = valid[n] ? (softmax(logits[n]) - onehot(targets[n])) * factor * upstream : exactly 0
 *
 * stats: float[4] on the device = {count, factor, upstream * factor (written by pdnl_linear_ce_backward_f32), unused}.  The
 * host never reads it: a step captured in a hipGraph follows a targets buffer whose mask changes between replays.  Counts and
 * sums are formed by one workgroup in a fixed order.  A valid target outside [0, V) raises *err_flag and is treated as 0;
 * negative targets do not wrap. */
#ifndef PDN_LOSS_H
#define PDN_LOSS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the unfused node: masked forms of pdn_cross_entropy_fwd_f32 / _fwd_bwd_f32 / _bwd_f32 (nn/functional.py:364-381, no
 * counterpart).  Rows of 4096 <= V <= 32768 floats with V % 4 == 0 are held in registers, others are re-read from L2.
 * loss_row / lse_row: (rows,) scratch; an ignored row leaves 0 in both. */
int pdnl_cross_entropy_fwd_f32(const float* logits, const int64_t* targets, int64_t ignore_index, int64_t rows, int V, int mean,
                               float* loss_row, float* lse_row, float* loss_out, float* stats, int* err_flag, void* stream);
/* bytes of workspace for the fused column sums of dlogits (0: this shape has no such fusion); nn/functional.py:364-381, no
 * counterpart */
int64_t pdnl_cross_entropy_colsum_workspace_bytes(int64_t rows, int V);
/* forward and dlogits (already multiplied by factor; the caller applies the upstream scalar) in one pass; dlogits_colsum
 * (V floats, may be NULL) = column sums of dlogits, the bias gradient of the Linear that made the logits
 * (nn/functional.py:364-381, no counterpart) */
int pdnl_cross_entropy_fwd_bwd_f32(const float* logits, const int64_t* targets, int64_t ignore_index, int64_t rows, int V, int mean,
                                   float* loss_row, float* lse_row, float* loss_out, float* stats, float* dlogits,
                                   float* dlogits_colsum, void* workspace, int64_t workspace_bytes, int* err_flag, void* stream);
/* dlogits from the saved lse_row and stats of a forward pass; upstream: device scalar, NULL = 1 (nn/functional.py:364-381, no
 * counterpart) */
int pdnl_cross_entropy_bwd_f32(const float* logits, const int64_t* targets, int64_t ignore_index, const float* lse_row,
                               const float* upstream, const float* stats, float* dlogits, int64_t rows, int V, void* stream);

/* ---- the lm_head + loss node (nn/functional.py:364-381 behind llm/llama/model.py:179, no counterpart).
 * The finish after the projection, in the place of pdn_cross_entropy_from_lse_f32: from the rows' log-sum-exp it forms the
 * loss, the count and the factor, and prepares the backward: targets_safe[n] = targets[n], or V for an ignored row, and
 * lse[n] = +inf for an ignored row (written IN PLACE), with which both terms of dlogits the products form,
 * exp(logit - lse) and [column == target], are exactly 0 on that row. */
int pdnl_linear_ce_finish_f32(const float* logits, int64_t ldl, float* lse, const int64_t* targets, int64_t ignore_index,
                              int64_t rows, int V, int mean, float* loss_row, float* loss_out, float* stats,
                              int64_t* targets_safe, int* err_flag, void* stream);
/* The masked backward, in the place of pdn_linear_ce_backward_f32 and under its shape rules, alignment and workspace size
 * (pdn_linear_ce_workspace_bytes; the split-fp16 weight gradient is taken when the workspace holds its region, as there).
 * lse_masked / targets_safe / stats: what pdnl_linear_ce_finish_f32 left.  dx (rows x in_features, may be NULL): the input
 * gradient, rows of ignored tokens exactly 0; nothing is folded into it.  dx_deferred (may be NULL, exclusive with dx): the
 * product pdn_linear_ce_dx_deferred_f32 (or its split form) left in the forward pass with gscale 1 -- multiplied in place by
 * upstream * factor, rows of ignored tokens set to exactly 0.  dW / dbias as in pdn_linear_ce_backward_f32.
 * (nn/functional.py:364-381, no counterpart) */
int pdnl_linear_ce_backward_f32(const float* x, int64_t ldx, const float* logits, const float* lse_masked,
                                const int64_t* targets_safe, float* stats, const float* upstream, const float* W, float* dx,
                                float* dx_deferred, float* dW, float dw_beta, float* dbias, float db_beta, int64_t rows, int V,
                                int in_features, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
