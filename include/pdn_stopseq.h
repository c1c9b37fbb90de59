/* Multi-token stop sequences of a decode step -- Llama generation with stop_sequences: extensions of the pdnhip C ABI
 * (csrc/stop_seq.hip), exported by libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.
 * Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnh_) of their own: as for include/pdn_fsm.h and the headers before it -- the tests hold
 * each header, the library's exports under its prefix and the closed registry of the host emulation equal.  This header is
 * listed in _lib.STOPSEQ_HEADER_PATHS and held to the same three-way equality by tests/test_stopseq_abi_cpu.py: the
 * library's pdnh_* exports, and the emulation in tests/abi_emulator/_stopseq.py with its own NOT_EMULATED.
 *
 * Statement: pydynet_amd/llm/stop_sequences.py (the reference's generation, llm/llama/model.py:258-269, stops on nothing:
 * no entry below has a counterpart).  The sets of a call, CSR: set_off (n_sets + 1,) indexes into seq_off (n_seqs + 1,),
 * which indexes into toks (n_toks,), int32 each; a sequence holds 1 .. 16 tokens (any other length never matches) and
 * the first 16 sequences of a set are looked at.
 * A plan row's state: set[b], its set id (-1, or any id outside [0, n_sets): none); start[b], the position of its first
 * generated token (its prompt length); tail[b] (16 int32), a ring of its last generated tokens -- y_j, the j-th token the
 * request generated, at slot j & 15 (-1: nothing there).
 * For row b at position p = pos[b] behind the tick, with g = p - start[b] (the tick moved the row behind y_g = ids[b]):
 * p < 0, no set, or g < 1: nothing of the row is written.  Otherwise tail[b][g & 15] = ids[b], and when a sequence q of
 * the row's set, of length l <= g, equals y_{g-l+1} .. y_g and g > *min_new: pos[b] = -1 -- the row is stopped exactly as
 * the tick stops one on a stop id.
 * Nothing is allocated or read back inside a call, there are no atomics, and the tables are only read: a step that
 * contains pdnh_stop_step replays from a hipGraph while pdnh_stop_reset changes rows between replays.  Each launching
 * entry counts once in launch counter slot 53. */
#ifndef PDN_STOPSEQ_H
#define PDN_STOPSEQ_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Rows rows[i], i < n_rows (rows outside [0, B) are skipped) of the state take set = src_set[i], start = src_start[i]
 * (the row's prompt length) and a cleared tail (-1 in every slot); src_first[i] >= 0: the request's first token, which the
 * host already has, as y_1 (slot 1); -1: it will come out of a replayed step.  One launch, stream-ordered behind the
 * steps queued before it; the other rows are not written (no counterpart). */
int pdnh_stop_reset(int* set, int* start, int* tail, int B, const int* rows, int n_rows, const int* src_set,
                    const int* src_start, const int* src_first, void* stream);
/* The step's form, the last launch of a step (behind the tick and the logprobs tick): ids (B,) the tokens the tick
 * stored, pos (B,) the positions it left; min_new: one int32 in device memory, the call's min_new_tokens.  One wave per
 * row, 4 rows per workgroup; only pos[b] and tail[b] of rows that match / run are written (no counterpart). */
int pdnh_stop_step(const int64_t* ids, int* pos, int B, const int* set_off, const int* seq_off, const int* toks,
                   int n_sets, int n_seqs, int n_toks, const int* set, const int* start, int* tail, const int* min_new,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif
