/* Per-request logit edits of a decode step -- allowed_token_ids, logit_bias, min_new_tokens: extensions of the pdnhip C ABI
 * (csrc/logit_edit.hip), exported by libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.
 * Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdne_) of their own: as for include/pdn_optim.h, include/pdn_loss.h, include/pdn_segattn.h,
 * include/pdn_rowloss.h and include/pdn_smoothloss.h -- the tests hold each header, the library's exports under its prefix
 * and the closed registry of the host emulation equal.  This header is listed in _lib.EDIT_HEADER_PATHS and held to the same
 * three-way equality by tests/test_logitedit_abi_cpu.py: the library's pdne_* exports, and the emulation in
 * tests/abi_emulator/_logitedit.py with its own NOT_EMULATED.
 *
 * Statement: pydynet_amd/llm/logit_edits.py (the reference's generation, llm/llama/model.py:258-269, edits no logits: no
 * entry below has a counterpart).  For row b's fp32 logits z (V of them, rows `row_stride` floats apart, columns past V
 * never touched) with g = the number of tokens the row has generated, in this order:
 *   1. allow_on[b] != 0: z[v] = -inf for every v whose bit is clear in allow[b] (ceil(V / 32) words, bit v & 31 of word
 *      v >> 5);
 *   2. for each of the bias_n[b] entries (bias_ids[b][j], bias_val[b][j]) of row b's table (PDNE_MAX_BIAS entries per row,
 *      sorted by id, ids distinct and in [0, V)): z[id] = -inf where the value is -inf, else z[id] + value -- one fp32
 *      rounding;
 *   3. g < params->min_new_tokens: z[v] = -inf for every v whose bit is set in `stop` (ceil(V / 32) words, shared by the
 *      rows: the stop bitmask of the ragged and slot ticks).
 * cand_v / cand_i ((B, pdne_logit_edit_chunks(V)), both or neither): each 1024-token chunk's first maximum of the edited row
 * and its index -- the candidates the pick ticks reduce, n_blocks = pdne_logit_edit_chunks(V); as in csrc/penalty.hip a
 * NaN never wins against a number, and a chunk of nothing but NaN yields (NaN, its first index), numpy.argmax's answer for
 * a row of NaNs.  A row at a position < 0 is left untouched, its candidates too.
 * Nothing is allocated or read back inside a call, and the state is only read by the step: a step that contains
 * pdne_logit_edit_step_f32 replays from a hipGraph while pdne_logit_edit_reset changes the state between replays.  Each
 * launching entry counts once in launch counter slot 48. */
#ifndef PDN_LOGITEDIT_H
#define PDN_LOGITEDIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PDNE_MAX_BIAS 1024 /* bias entries per row: a row's table is staged in LDS (8 KiB) */

typedef struct pdne_logit_edit_params {
  int min_new_tokens;
  int reserved[3];
} pdne_logit_edit_params;

/* the vocabulary chunks of a row, ceil(V / 1024), one workgroup each: the width of cand_v / cand_i (no counterpart) */
int pdne_logit_edit_chunks(int V);
/* Rows rows[i], i < n_rows (rows outside [0, B) are skipped) of the state (allow (B, ceil(V / 32)), allow_on (B,), bias_ids /
 * bias_val (B, PDNE_MAX_BIAS), bias_n (B,), start (B,)) take entry i of the sources: src_allow (n_rows, ceil(V / 32)) with
 * src_allow_on (n_rows,) -- both NULL: no allowed set, allow_on = 0; a row with src_allow_on[i] == 0 keeps its old bits,
 * which nothing reads -- src_bias_ids / src_bias_val (n_rows, PDNE_MAX_BIAS) with src_bias_n (n_rows,) -- all NULL: empty
 * tables -- and src_start (n_rows,), the row's prompt length.  One launch, stream-ordered behind the steps queued before
 * it; the other rows' state is not written (no counterpart). */
int pdne_logit_edit_reset(unsigned* allow, int* allow_on, int* bias_ids, float* bias_val, int* bias_n, int* start, int B,
                          int V, const int* rows, int n_rows, const unsigned* src_allow, const int* src_allow_on,
                          const int* src_bias_ids, const float* src_bias_val, const int* src_bias_n, const int* src_start,
                          void* stream);
/* The step's form, between the vocabulary projection (or pdn_penalty_step_f32) and the tick: row b sits at pos[b]
 * (pos_per_row == 0: every row at pos[0], the rectangular step), g = pos - start[b]; the state of a plan as the reset left
 * it, `stop` the tick's own bitmask (NULL: no stop ids) (no counterpart). */
int pdne_logit_edit_step_f32(float* logits, int64_t row_stride, int B, int V, const pdne_logit_edit_params* params,
                             const unsigned* allow, const int* allow_on, const int* bias_ids, const float* bias_val,
                             const int* bias_n, const int* start, const int* pos, int pos_per_row, const unsigned* stop,
                             float* cand_v, int* cand_i, void* stream);
/* The same without a plan (prompt passes, the generic steps): every state pointer may be NULL (allow with allow_on, the
 * three of the bias table, stop: that edit is off), g = generated[b] (NULL: 0), pos (B,) only marks the rows to skip
 * (NULL: none) (no counterpart). */
int pdne_logit_edit_rows_f32(float* logits, int64_t row_stride, int B, int V, const pdne_logit_edit_params* params,
                             const unsigned* allow, const int* allow_on, const int* bias_ids, const float* bias_val,
                             const int* bias_n, const int* generated, const int* pos, const unsigned* stop, float* cand_v,
                             int* cand_i, void* stream);

#ifdef __cplusplus
}
#endif
#endif
