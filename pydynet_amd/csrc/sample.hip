// Sampled next token: temperature, top-k and top-p (nucleus) over full fp32 logit rows -- the generalisation of the
// greedy pick of llm/llama/model.py:258-269 (argmax(-1)) that `Llama.generate(..., temperature > 0)` runs.
//
// Contract (pydynet_amd/llm/sampling.py states it in NumPy; include/pdn_hip.h): for one row z of V logits and
// temperature T > 0
//   1. top-k: keep every token with z_i >= z_(k), the k-th largest value counting repeats (k = 0 or k >= V: off);
//   2. p_i = exp((z_i - max z) / T) over the kept tokens, normalised;
//   3. top-p: theta = the largest kept value whose mass of {kept i : z_i >= theta} is at least top_p; keep those
//      (top_p >= 1: off);
//   3b. min_p (the block's float at offset 12; 0: off; the per-row launches of include/pdn_persample.h only): a token kept
//       so far stays iff exp((z_i - max z) / T) >= min_p;
//   4. u = (w >> 40) * 2^-24 with w the first word of Philox4x64-10(counter (t, b, 0, 0), key (seed, 0)); the token is
//      the smallest id whose inclusive cumulative probability (ascending ids, kept tokens only) is greater than u.
//
// One workgroup of 1024 threads per row.  Every pass reads the row from global memory (a 32000-token row is 125 KB:
// L2-resident after the first pass, and the 32 KB histogram below leaves no room to stage it in LDS too).
// Determinism: no float is ever summed in an order that depends on timing.  The probability mass is carried as an
// integer -- w_i = round-down(exp((z_i - max) / T) * 2^40), at most 2^40 per token, so a 2^23-token row cannot
// overflow 64 bits -- and integer sums are exact whatever their order, LDS atomics included.  So both thresholds and
// the draw are exact functions of those integers: two launches on one input give the same ids.
//   * max: wave / block reductions (first maximum, the fallback token for degenerate rows);
//   * thresholds: radix select on order-preserving uint keys of the logits, 12 + 12 + 8 bits, one 4096-bin histogram
//     (counts for top-k, masses for top-p) per level, scanned from the top bin down;
//   * draw: each thread sums a contiguous chunk of ids, a block-wide inclusive scan of the chunk sums, and the thread
//     whose chunk holds the target walks it.
#include "sample_row.h"

// PER (include/pdn_persample.h): row b uses parameter block prm[b], is drawn with counter (pos[b], req ? req[b] : b) and
// is left alone at pos[b] < 0 (its block is not read); else every row uses *prm and counter (t, b).
template <bool PER>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(const float* __restrict__ logits, int64_t rs, int V,
                                                                 const SampleParams* __restrict__ prm, int64_t t,
                                                                 const int* __restrict__ pos, const int* __restrict__ req,
                                                                 int64_t* __restrict__ out) {
  __shared__ SmpShared s;
  const int b = blockIdx.x;
  if (PER) {
    const int pb = pos[b];
    if (pb < 0) return;                              // (uniform)
    const int tok = smp_row<true>(logits + (int64_t)b * rs, V, prm[b], (uint64_t)pb, (uint64_t)(req ? req[b] : b), s);
    if (threadIdx.x == 0) out[b] = tok;
    return;
  }
  const int tok = smp_row(logits + (int64_t)b * rs, V, *prm, (uint64_t)t, (uint64_t)b, s);
  if (threadIdx.x == 0) out[b] = tok;
}

extern "C" int pdn_sample_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params, int64_t t,
                                   int64_t* out_ids, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && out_ids && B > 0 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "pdn_sample_rows_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  PDN_CHECK_ARG(t >= 0, "pdn_sample_rows_f32: negative counter %lld", (long long)t);
  hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                     (const SampleParams*)params, t, nullptr, nullptr, out_ids);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  return PDN_OK;
}

// include/pdn_persample.h: the standalone draw with a parameter block, a position and (req != NULL) a counter id per row
extern "C" int pdnq_sample_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                    const int* pos, const int* req, int64_t* out_ids, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && pos && out_ids && B > 0 && B <= 65535 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "pdnq_sample_rows_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                     (const SampleParams*)params, (int64_t)0, pos, req, out_ids);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_PERSAMPLE);
  return PDN_OK;
}

// ---- the sampled form of pdn_decode_pick_tick_f32 (csrc/decode.hip): the last launch of a sampled decode step ---------
// ONE workgroup walks the B rows (B <= 8 on the graph path), so that "read *pos, then advance it" is race free; each row
// is drawn with counter (*pos, b).  Token b goes to ids[b], to the history slot (*hist)[*pos * B + b] and its embedding
// row to x_next[b], exactly as the greedy pick does.
// ROWS: the per-row form of decode_pick_tick_kernel<true> (csrc/decode.hip): row b is drawn with counter (pos[b], b),
// the history slot is (*hist)[*step * B + b] (-1 for a stopped row, pos[b] < 0, which is otherwise left alone), a
// token in the stop bitmask stops its row (pos[b] = -1), else pos[b] += 1; then *step += 1.
// SLOTS (with ROWS; Llama.serve): row b is drawn with counter (pos[b], req[b]) -- the request it holds, not the row --,
// the history is a ring of `ring` steps, (*hist)[(*step % ring) * B + b], and left[b] counts the tokens row b may still
// produce: a live row stores left[b] - 1 and stops once it reaches 0.
// PER (with ROWS; include/pdn_persample.h): row b uses parameter block prm[b], read by every thread before the barriers of
// smp_row like pos[b]; a stopped row's block is not read.
template <bool ROWS, bool SLOTS = false, bool PER = false>
__global__ __launch_bounds__(SMP_THREADS) void decode_sample_tick_kernel(
    const float* __restrict__ logits, int64_t rs, int B, int V, const SampleParams* __restrict__ prm,
    int64_t* __restrict__ ids, int* __restrict__ pos, int64_t* const* __restrict__ hist, const float* __restrict__ emb,
    int64_t emb_rs, int D, float* __restrict__ x_next, int* __restrict__ step, const unsigned* __restrict__ stop,
    const int* __restrict__ req, int* __restrict__ left, int ring) {
  __shared__ SmpShared s;
  const int tid = threadIdx.x;
  const int p = ROWS ? *step : (pos ? *pos : 0);
  const SampleParams pr0 = PER ? SampleParams{} : *prm;
  int64_t* hrow = hist ? *hist + (int64_t)(SLOTS ? p % ring : p) * B : nullptr;
  for (int b = 0; b < B; ++b) {
    const int pb = ROWS ? pos[b] : p;      // (read by every thread before the barriers of smp_row)
    if (ROWS && pb < 0) {                  // (uniform)
      if (tid == 0 && hrow) __hip_atomic_store(hrow + b, (int64_t)-1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      continue;
    }
    const SampleParams pr = PER ? prm[b] : pr0;
    const int64_t tok = smp_row<PER>(logits + (int64_t)b * rs, V, pr, (uint64_t)pb, (uint64_t)(SLOTS ? req[b] : b), s);
    if (tid == 0) {
      ids[b] = tok;
      if (hrow) __hip_atomic_store(hrow + b, tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (may be host memory)
      if (SLOTS) {
        const int lb = left[b] - 1;
        left[b] = lb;
        pos[b] = (lb <= 0 || (stop && ((stop[tok >> 5] >> (tok & 31)) & 1u))) ? -1 : pb + 1;
      } else if (ROWS) {
        pos[b] = (stop && ((stop[tok >> 5] >> (tok & 31)) & 1u)) ? -1 : pb + 1;
      }
    }
    if (emb) {
      const float* er = emb + tok * emb_rs;
      for (int d = tid; d < D; d += SMP_THREADS) x_next[(int64_t)b * D + d] = er[d];
    }
  }
  if (ROWS) {
    __syncthreads();                       // (every thread has read *step)
    if (tid == 0) *step = p + 1;
    return;
  }
  // every thread read *pos before the first barrier of smp_row
  if (tid == 0 && pos) *pos = p + 1;
}

extern "C" int pdn_decode_sample_tick_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                          int64_t* next_ids, int* pos, int64_t* const* history, const float* emb,
                                          int64_t emb_row_stride, int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && next_ids && B > 0 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "pdn_decode_sample_tick_f32: bad arguments (B %d, V %d)", B, V);
  PDN_CHECK_ARG(!history || pos, "pdn_decode_sample_tick_f32: a history needs the position");
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "pdn_decode_sample_tick_f32: an embedding table needs x_next and D");
  hipLaunchKernelGGL(decode_sample_tick_kernel<false>, dim3(1), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits,
                     row_stride, B, V, (const SampleParams*)params, next_ids, pos, history, emb, emb_row_stride, D, x_next,
                     nullptr, nullptr, nullptr, nullptr, 0);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  return PDN_OK;
}

// The same with a position per row (decode_sample_tick_kernel<true>): pos (B,) and step (1,) int32 are required.
// PER: the pdnq_ form, `params` = B blocks.
template <bool PER>
static int sample_tick_rows(const char* name, const float* logits, int64_t row_stride, int B, int V, const void* params,
                            int64_t* next_ids, int* pos, int* step, const unsigned* stop_mask, int64_t* const* history,
                            const float* emb, int64_t emb_row_stride, int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && next_ids && pos && step && B > 0 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "%s: bad arguments (B %d, V %d)", name, B, V);
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "%s: an embedding table needs x_next and D", name);
  hipLaunchKernelGGL((decode_sample_tick_kernel<true, false, PER>), dim3(1), dim3(SMP_THREADS), 0, (hipStream_t)stream,
                     logits, row_stride, B, V, (const SampleParams*)params, next_ids, pos, history, emb, emb_row_stride, D,
                     x_next, step, stop_mask, nullptr, nullptr, 0);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_DECODE_ROWS);
  if (PER) pdn_count(PDN_CNT_PERSAMPLE);
  return PDN_OK;
}

extern "C" int pdn_decode_sample_tick_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                               int64_t* next_ids, int* pos, int* step, const unsigned* stop_mask,
                                               int64_t* const* history, const float* emb, int64_t emb_row_stride, int D,
                                               float* x_next, void* stream) {
  return sample_tick_rows<false>("pdn_decode_sample_tick_rows_f32", logits, row_stride, B, V, params, next_ids, pos, step,
                                 stop_mask, history, emb, emb_row_stride, D, x_next, stream);
}

extern "C" int pdnq_decode_sample_tick_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                                int64_t* next_ids, int* pos, int* step, const unsigned* stop_mask,
                                                int64_t* const* history, const float* emb, int64_t emb_row_stride, int D,
                                                float* x_next, void* stream) {
  return sample_tick_rows<true>("pdnq_decode_sample_tick_rows_f32", logits, row_stride, B, V, params, next_ids, pos, step,
                                stop_mask, history, emb, emb_row_stride, D, x_next, stream);
}

// The per-row tick of a served batch (decode_sample_tick_kernel<true, true>): as pdn_decode_sample_tick_rows_f32, but
// row b is drawn with counter (pos[b], req[b]), left (B,) int32 counts the tokens row b may still produce and the
// history is a ring of `ring` steps, (*history)[(*step % ring) * B + b].
// PER: the pdnq_ form, `params` = B blocks.
template <bool PER>
static int sample_tick_slots(const char* name, const float* logits, int64_t row_stride, int B, int V, const void* params,
                             int64_t* next_ids, int* pos, int* step, const int* req, int* left, int ring,
                             const unsigned* stop_mask, int64_t* const* history, const float* emb, int64_t emb_row_stride,
                             int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && next_ids && pos && step && req && left && ring > 0 && B > 0 && V > 0 &&
                    V <= (1 << 23) && row_stride >= V,
                "%s: bad arguments (B %d, V %d, ring %d)", name, B, V, ring);
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "%s: an embedding table needs x_next and D", name);
  hipLaunchKernelGGL((decode_sample_tick_kernel<true, true, PER>), dim3(1), dim3(SMP_THREADS), 0, (hipStream_t)stream,
                     logits, row_stride, B, V, (const SampleParams*)params, next_ids, pos, history, emb, emb_row_stride, D,
                     x_next, step, stop_mask, req, left, ring);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_DECODE_SLOTS);
  if (PER) pdn_count(PDN_CNT_PERSAMPLE);
  return PDN_OK;
}

extern "C" int pdn_decode_sample_tick_slots_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                                int64_t* next_ids, int* pos, int* step, const int* req, int* left,
                                                int ring, const unsigned* stop_mask, int64_t* const* history,
                                                const float* emb, int64_t emb_row_stride, int D, float* x_next,
                                                void* stream) {
  return sample_tick_slots<false>("pdn_decode_sample_tick_slots_f32", logits, row_stride, B, V, params, next_ids, pos,
                                  step, req, left, ring, stop_mask, history, emb, emb_row_stride, D, x_next, stream);
}

extern "C" int pdnq_decode_sample_tick_slots_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                                 int64_t* next_ids, int* pos, int* step, const int* req, int* left,
                                                 int ring, const unsigned* stop_mask, int64_t* const* history,
                                                 const float* emb, int64_t emb_row_stride, int D, float* x_next,
                                                 void* stream) {
  return sample_tick_slots<true>("pdnq_decode_sample_tick_slots_f32", logits, row_stride, B, V, params, next_ids, pos,
                                 step, req, left, ring, stop_mask, history, emb, emb_row_stride, D, x_next, stream);
}
