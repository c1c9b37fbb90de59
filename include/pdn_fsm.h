/* Token-FSM constrained decoding of a decode step -- Llama generation with token_fsm: extensions of the pdnhip C ABI
 * (csrc/token_fsm.hip), exported by libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.
 * Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnf_) of their own: as for include/pdn_logitedit.h and the headers before it -- the tests
 * hold each header, the library's exports under its prefix and the closed registry of the host emulation equal.  This
 * header is listed in _lib.FSM_HEADER_PATHS and held to the same three-way equality by tests/test_fsm_abi_cpu.py: the
 * library's pdnf_* exports, and the emulation in tests/abi_emulator/_fsm.py with its own NOT_EMULATED.
 *
 * Statement: pydynet_amd/llm/token_fsm.py (the reference's generation, llm/llama/model.py:258-269, constrains nothing: no
 * entry below has a counterpart).  The machines, CSR over S states and E edges: offsets (S + 1,), tokens (E,) ascending
 * within a state, next (E,), dflt (S,) (-1: no default), int32 each.  A state s in [0, S) allows its tokens, or every
 * token when dflt[s] >= 0; any other state value (-1: off) masks nothing and never advances.  advance(s, t) = next[j]
 * where tokens[j] == t within s, else dflt[s] when >= 0, else s.
 * A plan row's state is one 64-bit word, ((int64_t)position << 32) | (uint32_t)state: the state the row is in at that
 * position.  For row b at position p (p < 0: logits, word and candidates untouched) with g = p - start[b]:
 *   cur = start_state[b]                 when g <= 0,
 *         the word's state               when the word's position is p,
 *         advance(the word's state, ids[b])   otherwise;
 * the word becomes (p, cur), and z[v] = -inf for every v < V that cur does not allow (rows `row_stride` floats apart,
 * columns past V never touched).
 * cand_v / cand_i ((B, pdnf_fsm_chunks(V)), both or neither): each 1024-token chunk's first maximum of the masked row and
 * its index -- the candidates the pick ticks reduce; as in csrc/penalty.hip a NaN never wins against a number, and a chunk
 * of nothing but NaN yields (NaN, its first index).
 * Nothing is allocated or read back inside a call, there are no atomics, and the tables are only read: a step that
 * contains pdnf_fsm_step_f32 replays from a hipGraph while pdnf_fsm_reset changes rows between replays.  Each launching
 * entry counts once in launch counter slot 52. */
#ifndef PDN_FSM_H
#define PDN_FSM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the vocabulary chunks of a row, ceil(V / 1024), one workgroup each: the width of cand_v / cand_i (no counterpart) */
int pdnf_fsm_chunks(int V);
/* Rows rows[i], i < n_rows (rows outside [0, B) are skipped) of the state take start_state = src_state[i], start =
 * src_start[i] (the row's prompt length) and the word (src_start[i], src_state[i]).  One launch, stream-ordered behind
 * the steps queued before it; the other rows are not written (no counterpart). */
int pdnf_fsm_reset(int64_t* state, int* start_state, int* start, int B, const int* rows, int n_rows, const int* src_state,
                   const int* src_start, void* stream);
/* The step's form, between pdn_penalty_step_f32 (or the vocabulary projection) and pdne_logit_edit_step_f32 (or the
 * tick): row b sits at pos[b] (pos_per_row == 0: every row at pos[0], the rectangular step) and is fed ids[b]; the state
 * of a plan as the reset left it.  Every workgroup of a row works out cur for itself and only the one of chunk 0 stores
 * the word, with one 8-byte store: whichever of the two words another workgroup reads, it arrives at the same cur (no
 * counterpart). */
int pdnf_fsm_step_f32(float* logits, int64_t row_stride, int B, int V, const int* offsets, const int* tokens,
                      const int* next, const int* dflt, int S, int E, int64_t* state, const int* start_state,
                      const int* start, const int64_t* ids, const int* pos, int pos_per_row, float* cand_v, int* cand_i,
                      void* stream);
/* The same without a plan (prompt passes, the generic steps): row b is masked for states[b], which is only read; pos (B,)
 * only marks the rows to skip (NULL: none) (no counterpart). */
int pdnf_fsm_rows_f32(float* logits, int64_t row_stride, int B, int V, const int* offsets, const int* tokens,
                      const int* dflt, int S, int E, const int* states, const int* pos, float* cand_v, int* cand_i,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
