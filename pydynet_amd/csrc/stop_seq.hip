// Multi-token stop sequences of a decode step (Llama.generate_ragged / serve with stop_sequences); the contract is stated in
// NumPy in llm/stop_sequences.py, the ABI in include/pdn_stopseq.h.  The sets of a call are CSR tables the kernels only
// read: set_off (n_sets + 1) into seq_off (n_seqs + 1) into toks (n_toks).  Row state, per plan: set (B,), the row's set id
// (-1: none); start (B,), the position of the row's first generated token (its prompt length); tail (B, 16), a ring of
// the row's last generated tokens -- y_j, the j-th token the request generated, at slot j & 15.
//
//   stop_reset_kernel  one thread per listed row: its set, prompt length, a cleared tail and (when given) its first token.
//   stop_step_kernel   the last launch of a step, behind the tick: one wave per row, 4 rows per workgroup.  A row the
//                      tick left at pos < 0 (stopped, empty, mid-prompt) or without a set is untouched.  Any other row has
//                      just stored y_g = ids[b] and moved to position start + g: lane q walks sequence q of the row's set
//                      backwards through the ring (its last token against ids[b], which no lane reads from the ring), a
//                      wave ballot combines the lanes, and lane 0 stores y_g into the ring and, on a match at g > min_new,
//                      pos[b] = -1 -- all a stop is on the device (the ROWS / SLOTS branches of the ticks).
// No atomics, no LDS, nothing allocated or read back: a step that contains the launch replays from a hipGraph.
#include "common.h"

#define PDNH_MAX_LEN 16                  // tokens of a sequence = slots of a row's ring
#define PDNH_MAX_SEQS 16                 // sequences of a set looked at: one lane each
#define SS_THREADS 256
#define SS_ROWS (SS_THREADS / 64)        // one wave per row

__global__ __launch_bounds__(SS_THREADS) void stop_reset_kernel(
    int* __restrict__ set, int* __restrict__ start, int* __restrict__ tail, int B, const int* __restrict__ rows, int n_rows,
    const int* __restrict__ src_set, const int* __restrict__ src_start, const int* __restrict__ src_first) {
  const int i = blockIdx.x * SS_THREADS + threadIdx.x;
  if (i >= n_rows) return;
  const int b = rows[i];
  if (b < 0 || b >= B) return;
  set[b] = src_set[i];
  start[b] = src_start[i];
  const int first = src_first[i];
  int* t = tail + (int64_t)b * PDNH_MAX_LEN;
#pragma unroll
  for (int j = 0; j < PDNH_MAX_LEN; ++j) t[j] = (j == 1 && first >= 0) ? first : -1;   // (y_1 at slot 1)
}

__global__ __launch_bounds__(SS_THREADS) void stop_step_kernel(
    const long long* __restrict__ ids, int* __restrict__ pos, int B, const int* __restrict__ set_off,
    const int* __restrict__ seq_off, const int* __restrict__ toks, int n_sets, int n_seqs, int n_toks,
    const int* __restrict__ set, const int* __restrict__ start, int* __restrict__ tail, const int* __restrict__ min_new) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SS_ROWS + (threadIdx.x >> 6);
  if (b >= B) return;                                  // (uniform per wave, as every exit below)
  const int p = pos[b], s = set[b];
  if (p < 0 || s < 0 || s >= n_sets) return;
  const int g = p - start[b];                          // the tick moved the row behind its g-th generated token
  if (g < 1) return;
  const long long t64 = ids[b];
  const int tok = (t64 < 0 || t64 > 0x7fffffffll) ? -1 : (int)t64;                       // (no sequence holds -1)
  int* t = tail + (int64_t)b * PDNH_MAX_LEN;
  const int q0 = min(max(set_off[s], 0), n_seqs), q1 = min(max(set_off[s + 1], q0), n_seqs);
  bool hit = false;
  if (lane < PDNH_MAX_SEQS && q0 + lane < q1) {
    const int lo = min(max(seq_off[q0 + lane], 0), n_toks), hi = min(max(seq_off[q0 + lane + 1], lo), n_toks);
    const int n = hi - lo;
    if (n >= 1 && n <= PDNH_MAX_LEN && n <= g) {
      hit = toks[hi - 1] == tok;
      for (int j = 1; j < n && hit; ++j) hit = toks[hi - 1 - j] == t[(g - j) & (PDNH_MAX_LEN - 1)];   // (never slot g & 15)
    }
  }
  const unsigned long long any = __ballot(hit);
  if (lane == 0) {
    t[g & (PDNH_MAX_LEN - 1)] = tok;
    if (any != 0ull && g > min_new[0]) pos[b] = -1;
  }
}

extern "C" int pdnh_stop_reset(int* set, int* start, int* tail, int B, const int* rows, int n_rows, const int* src_set,
                               const int* src_start, const int* src_first, void* stream) {
  if (n_rows == 0) return PDN_OK;
  PDN_CHECK_ARG(set && start && tail && rows && src_set && src_start && src_first && B > 0 && n_rows > 0,
                "pdnh_stop_reset: bad arguments (B %d, rows %d)", B, n_rows);
  hipLaunchKernelGGL(stop_reset_kernel, dim3((n_rows + SS_THREADS - 1) / SS_THREADS), dim3(SS_THREADS), 0,
                     (hipStream_t)stream, set, start, tail, B, rows, n_rows, src_set, src_start, src_first);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_STOP_SEQ);
  return PDN_OK;
}

extern "C" int pdnh_stop_step(const int64_t* ids, int* pos, int B, const int* set_off, const int* seq_off, const int* toks,
                              int n_sets, int n_seqs, int n_toks, const int* set, const int* start, int* tail,
                              const int* min_new, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(ids && pos && set_off && seq_off && toks && set && start && tail && min_new && B > 0 && n_sets > 0 &&
                    n_seqs > 0 && n_toks > 0,
                "pdnh_stop_step: bad arguments (B %d, sets %d, sequences %d, tokens %d)", B, n_sets, n_seqs, n_toks);
  hipLaunchKernelGGL(stop_step_kernel, dim3((B + SS_ROWS - 1) / SS_ROWS), dim3(SS_THREADS), 0, (hipStream_t)stream,
                     (const long long*)ids, pos, B, set_off, seq_off, toks, n_sets, n_seqs, n_toks, set, start, tail, min_new);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_STOP_SEQ);
  return PDN_OK;
}
