/* Cross entropy with label_smoothing and z_loss: extensions of the pdnhip C ABI (csrc/smooth_loss.hip), exported by
 * libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes,
 * pdn_last_error, streams, the error flag) are the core header's.
 *
 * Why a header and a prefix (pdnz_) of their own: as for include/pdn_optim.h, include/pdn_loss.h, include/pdn_segattn.h and
 * include/pdn_rowloss.h -- the tests hold each header, the library's exports under its prefix and the closed registry of the
 * host emulation equal.  This header is listed in _lib.SMOOTH_HEADER_PATHS and held to the same three-way equality by
 * tests/test_smoothloss_abi_cpu.py: the library's pdnz_* exports, and the emulation in tests/abi_emulator/_smoothloss.py with
 * its own NOT_EMULATED.
 *
 * Every entry below extends the cross entropy of nn/functional.py:364-381, which has neither argument, so there is no
 * counterpart.  Statement: pydynet_amd/core/fused/smooth_loss.py.
 *
 *   eps = label_smoothing in [0, 1], lam = z_loss >= 0
 *   valid[n] = !masked || targets[n] != ignore_index;   lse = logsumexp(logits[n]);   a = 1 + 2 lam lse
 *   row[n]   = valid[n] ? lse - (1 - eps) logits[n][t] - eps mean_v logits[n] + lam lse^2 : 0
 *   dlogits[n] = valid[n] ? u[n] (a softmax(logits[n]) - (1 - eps) onehot(t) - eps / V) : exactly 0, whatever u[n] holds
 *              = u'[n] (softmax - onehot) + c[n] onehot - e[n],   u' = u a,  c = u (2 lam lse + eps),  e = u eps / V
 *   reduction: 0 'none' (the value is row), 1 'sum', 2 'mean' (divided by the number of valid rows; none left: 0)
 *   the upstream number of a row: u[n] where a (rows,) vector u is given, else upstream[0] * stats[1] (either NULL: 1)
 *
 * A valid target outside [0, V) raises *err_flag; negative targets do not wrap.  Nothing is read back by the host, every
 * sum is formed in a fixed order without atomics, nothing is allocated inside a call: a step built on these entries replays
 * from a hipGraph over changing targets.  Each entry counts once in launch counter slot 45. */
#ifndef PDN_SMOOTHLOSS_H
#define PDN_SMOOTHLOSS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the unfused node (nn/functional.py:364-381, no counterpart).  One pass over each row yields its maximum, sum of
 * exponentials and sum together; loss_row and lse_row (0 on ignored rows) are left for the backward.  reduction 1 / 2:
 * loss_out[0] and stats = {count, factor} (4 floats), kept on the device as pdnl_cross_entropy_fwd_f32 does; reduction 0:
 * loss_out and stats may be NULL.  Rows of 4096 <= V <= 32768 floats with V % 4 == 0 and aligned rows pass through
 * registers, a 1024-thread workgroup per row, others are streamed (float4 where the row's address allows it); both walk on
 * past the grid. */
int pdnz_cross_entropy_fwd_f32(const float* logits, const int64_t* targets, int masked, int64_t ignore_index, int64_t rows,
                               int V, int reduction, float label_smoothing, float z_loss, float* loss_row, float* lse_row,
                               float* loss_out, float* stats, int* err_flag, void* stream);
/* dlogits as above from the saved lse_row; an ignored row is zero-filled by a select.  u: (rows,) or NULL; upstream: one
 * float on the device or NULL; stats: what the forward left, or NULL.  The same two row variants
 * (nn/functional.py:364-381, no counterpart). */
int pdnz_cross_entropy_bwd_f32(const float* logits, const int64_t* targets, int masked, int64_t ignore_index,
                               const float* lse_row, const float* u, const float* upstream, const float* stats,
                               float label_smoothing, float z_loss, float* dlogits, int64_t rows, int V, void* stream);

/* ---- the lm_head + loss node (nn/functional.py:364-381 behind llm/llama/model.py:179, no counterpart).
 * wsum[k] = sum_v W[k][v] for k < in_features and wsum[in_features] = sum_v bias[v] (bias NULL: 0), W (in_features x V)
 * contiguous: mean_v logits[n] = (x[n] . wsum[:in_features] + wsum[in_features]) / V needs no pass over the logits. */
int pdnz_weight_sums_f32(const float* W, const float* bias, int in_features, int V, float* wsum, void* stream);
/* The finish after the projection: loss_row[n] = row[n] from the lse the projection or the deferred product left, the
 * gathered target logit and x[n] . wsum (x and wsum may be NULL when label_smoothing == 0).  targets_safe and the masked
 * lse (written IN PLACE) exactly as pdnr_linear_ce_finish_rows_f32 leaves them: targets_safe[n] = targets[n], or V for an
 * ignored row (0, and *err_flag raised, for a valid one outside [0, V)); lse[n] = +inf for an ignored row.  reduction 1 / 2:
 * loss_out[0] and stats = {count, factor} as well (nn/functional.py:364-381, no counterpart). */
int pdnz_linear_ce_finish_f32(const float* logits, int64_t ldl, float* lse, const int64_t* targets, int masked,
                              int64_t ignore_index, const float* x, int64_t ldx, const float* wsum, int64_t rows, int V,
                              int in_features, int reduction, float label_smoothing, float z_loss, float* loss_row,
                              float* loss_out, float* stats, int64_t* targets_safe, int* err_flag, void* stream);
/* The row coefficient vectors u_out = u', c_out = c, e_out = e ((rows,) each), exactly 0 where targets_safe[n] == V.
 * u_out is the upstream vector pdnr_linear_ce_backward_rows_f32 is then called with (nn/functional.py:364-381, no
 * counterpart). */
int pdnz_row_coefficients_f32(const float* lse_masked, const int64_t* targets_safe, const float* u, const float* upstream,
                              const float* stats, float label_smoothing, float z_loss, int64_t rows, int V, float* u_out,
                              float* c_out, float* e_out, void* stream);
/* bytes of workspace of pdnz_linear_ce_corrections_f32 (nn/functional.py:364-381, no counterpart) */
int64_t pdnz_linear_ce_corrections_workspace_bytes(int64_t rows, int V, int in_features);
/* The two terms the products do not form, ADDED to what pdnr_linear_ce_backward_rows_f32 left (so dW and dbias carry its
 * dw_beta / db_beta already); each of dx, dW, dbias may be NULL.  e NULL (label_smoothing == 0): no uniform term.
 *   dx[n][:]  += c[n] W[:, t[n]] - e[n] wsum           (dx rows x in_features, contiguous; ignored rows stay exactly 0)
 *   dW[:, v]  += sum_{n: t[n] == v} c[n] x[n] - r,      r = sum_n e[n] x[n]
 *   dbias[v]  += sum_{n: t[n] == v} c[n]     - sum_n e[n]
 * The sums over the rows of a class: a workgroup owns a contiguous range of classes (at most 128, as many as an fp32
 * accumulator [classes][in_features + 1] of 56 KiB of LDS holds), walks ALL targets_safe in row order and adds the rows that
 * fall into its range -- no sort, no atomics, every sum in row order; r by a two-stage column sum (row slabs in the
 * workspace, then the slabs in their order).  in_features + 2 above 14336: PDN_EUNSUPPORTED
 * (nn/functional.py:364-381, no counterpart). */
int pdnz_linear_ce_corrections_f32(const float* x, int64_t ldx, const float* W, const float* wsum,
                                   const int64_t* targets_safe, const float* c, const float* e, float* dx, float* dW,
                                   float* dbias, int64_t rows, int V, int in_features, void* workspace,
                                   int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
