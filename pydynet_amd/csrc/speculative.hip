// Prompt-lookup speculative decoding (Llama.generate_ragged(speculate=k)); the contract is stated in NumPy in
// llm/speculative.py.  A target pass runs B * (k + 1) query rows: row b owns rows b (k + 1) .. b (k + 1) + k, which hold
// its last token t_0 and up to k draft tokens at consecutive cache positions.  Everything a pass needs lives on the device
// -- each row's token history, its position and its budget -- so passes replay back to back with no upload between them.
//
//   spec_draft_kernel        one workgroup per row: the n-gram lookup over the row's history, then the row's fed tokens,
//                            their positions (-1: an unused query row) and its run [first row, d + 1, pos, 0] in the
//                            layout of csrc/extend.hip.
//   spec_pick_kernel /       one workgroup per query row: the greedy pick over the vocabulary projection's block
//   spec_sample_kernel       candidates (lowest index on ties), or the draw of sample_row.h with counter (position, row).
//   spec_accept_kernel       ONE workgroup, a thread per row: the accept rule, stop ids and budget; appends the yielded
//                            tokens to the history, moves pos / left on, stores [count, drafted, accepted, tokens...] into
//                            the pass's mailbox slot and advances the pass counter.  A single workgroup orders all of it:
//                            no cross-workgroup protocol, no atomics.
#include "common.h"
#include "sample_row.h"

#define SP_NGRAM 3
#define SP_MAX_K 16
#define SP_THREADS 256

// grid B, SP_THREADS threads
__global__ __launch_bounds__(SP_THREADS) void spec_draft_kernel(const int* __restrict__ hist, int hist_stride,
                                                               const int* __restrict__ hlen, const int* __restrict__ pos,
                                                               const int* __restrict__ left, int k,
                                                               int64_t* __restrict__ tok, int* __restrict__ qpos,
                                                               int* __restrict__ runs) {
  __shared__ int wbest[SP_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K1 = k + 1, base = b * K1;
  const int p = hlen[b] >= 1 ? pos[b] : -1;
  if (p < 0) {                                   // (uniform) a stopped row: no run, every query row masked
    if (tid < K1) { tok[base + tid] = 0; qpos[base + tid] = -1; }
    if (tid == 0) { runs[4 * b] = base; runs[4 * b + 1] = 0; runs[4 * b + 2] = 0; runs[4 * b + 3] = 0; }
    return;
  }
  const int T = min(hlen[b], hist_stride);
  const int* h = hist + (int64_t)b * hist_stride;
  const int cap = min(k, left[b] - 1);
  // key of a match ending at e (exclusive, e < T): m << 24 | e, m = the longest n <= NGRAM with h[e-n:e] == h[T-n:T];
  // the maximum is the largest n that matches anywhere and, for it, the largest j = e - n
  int best = -1;
  if (cap > 0) {
    for (int e = 1 + tid; e < T; e += SP_THREADS) {
      int m = 0;
      while (m < SP_NGRAM && e - 1 - m >= 0 && h[e - 1 - m] == h[T - 1 - m]) ++m;
      if (m > 0) best = max(best, (m << 24) | e);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < SP_THREADS / 64; ++w) best = max(best, wbest[w]);
  const int e = best & 0xffffff;
  const int d = best >= 0 ? min(cap, T - e) : 0;
  if (tid < K1) {
    tok[base + tid] = tid == 0 ? h[T - 1] : (tid <= d ? h[e + tid - 1] : 0);
    qpos[base + tid] = tid <= d ? p + tid : -1;
  }
  if (tid == 0) { runs[4 * b] = base; runs[4 * b + 1] = d + 1; runs[4 * b + 2] = p; runs[4 * b + 3] = 0; }
}

// grid B (k + 1), 256 threads: the greedy pick of each live query row over its block candidates
__global__ __launch_bounds__(256) void spec_pick_kernel(const float* __restrict__ vals, const int* __restrict__ args,
                                                        int n, const int* __restrict__ qpos, int64_t* __restrict__ picks) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (qpos[r] < 0) return;                       // (uniform)
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int i = tid; i < n; i += 256) {
    const float v = vals[(int64_t)r * n + i];
    const int a = args[(int64_t)r * n + i];
    if (v > best || (v == best && a < idx)) { best = v; idx = a; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w)
      if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
    picks[r] = idx == 0x7fffffff ? 0 : idx;
  }
}

// grid B (k + 1), SMP_THREADS threads: the draw of sample.hip for each live query row, counter (its position, its row)
// PER (include/pdn_persample.h): query row r uses parameter block prm[r / K1], its row's, else *prm.
template <bool PER>
__global__ __launch_bounds__(SMP_THREADS) void spec_sample_kernel(const float* __restrict__ logits, int64_t rs, int V,
                                                                  const SampleParams* __restrict__ prm, int K1,
                                                                  const int* __restrict__ qpos,
                                                                  int64_t* __restrict__ picks) {
  __shared__ SmpShared s;
  const int r = blockIdx.x;
  const int p = qpos[r];
  if (p < 0) return;                             // (uniform)
  const int64_t t = smp_row<PER>(logits + (int64_t)r * rs, V, prm[PER ? r / K1 : 0], (uint64_t)p, (uint64_t)(r / K1), s);
  if (threadIdx.x == 0) picks[r] = t;
}

// one workgroup of SP_THREADS threads: thread b (and b + SP_THREADS ...) settles row b
__global__ __launch_bounds__(SP_THREADS) void spec_accept_kernel(const int64_t* __restrict__ tok,
                                                                 const int* __restrict__ qpos,
                                                                 const int64_t* __restrict__ picks, int B, int k,
                                                                 int* __restrict__ hist, int hist_stride,
                                                                 int* __restrict__ hlen, int* __restrict__ pos,
                                                                 int* __restrict__ left, const unsigned* __restrict__ stop,
                                                                 int* __restrict__ step, int64_t* const* __restrict__ mbox) {
  const int tid = threadIdx.x, K1 = k + 1, W = k + 4;
  const int s = *step;
  int64_t* slot = mbox && *mbox ? *mbox + (int64_t)s * B * W : nullptr;
  for (int b = tid; b < B; b += SP_THREADS) {
    const int pb = pos[b], base = b * K1;
    int64_t* out = slot ? slot + (int64_t)b * W : nullptr;
    int c = 0, d = 0, a = 0;
    if (pb >= 0) {
      while (d < k && qpos[base + d + 1] >= 0) ++d;
      while (a < d && picks[base + a] == tok[base + a + 1]) ++a;
      const int lb = left[b];
      c = min(a + 1, lb);
      bool hit = false;
      for (int i = 0; i < c; ++i) {
        const int64_t t = picks[base + i];
        if (stop && ((stop[t >> 5] >> (t & 31)) & 1u)) { c = i + 1; hit = true; break; }
      }
      const int T = hlen[b];
      int* hrow = hist + (int64_t)b * hist_stride;
      for (int i = 0; i < c; ++i)
        if (T + i < hist_stride) hrow[T + i] = (int)picks[base + i];
      hlen[b] = T + c;
      left[b] = lb - c;
      pos[b] = (hit || lb - c <= 0) ? -1 : pb + c;
    }
    if (out) {                                   // (mapped host memory: stores at system scope)
      __hip_atomic_store(out, (int64_t)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(out + 1, (int64_t)d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(out + 2, (int64_t)min(a, c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      for (int i = 0; i < K1; ++i)
        __hip_atomic_store(out + 3 + i, i < c ? picks[base + i] : (int64_t)-1, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __syncthreads();                               // (every thread has read *step)
  if (tid == 0) *step = s + 1;
}

extern "C" int pdn_spec_draft_rows(const int* hist, int hist_stride, const int* hist_len, const int* pos, const int* left,
                                   int B, int k, int64_t* tokens, int* qpos, int* runs, void* stream) {
  PDN_CHECK_ARG(hist && hist_len && pos && left && tokens && qpos && runs && B > 0 && k >= 0 && k <= SP_MAX_K &&
                    (int64_t)B * (k + 1) <= 65535 && hist_stride > 0 && hist_stride < (1 << 24),
                "pdn_spec_draft_rows: bad arguments (B %d, k %d, history stride %d)", B, k, hist_stride);
  hipLaunchKernelGGL(spec_draft_kernel, dim3(B), dim3(SP_THREADS), 0, (hipStream_t)stream, hist, hist_stride, hist_len,
                     pos, left, k, tokens, qpos, runs);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SPECULATE);
  return PDN_OK;
}

#define SP_TICK_CHECK(name)                                                                                            \
  PDN_CHECK_ARG(tokens && qpos && picks && hist && hist_len && pos && left && step && B > 0 && k >= 0 &&              \
                    k <= SP_MAX_K && (int64_t)B * (k + 1) <= 65535 && hist_stride > 0,                                 \
                name ": bad arguments (B %d, k %d, history stride %d)", B, k, hist_stride)

extern "C" int pdn_spec_verify_pick_tick_f32(const float* blk_max, const int* blk_arg, int n_blocks,
                                             const int64_t* tokens, const int* qpos, int B, int k, int64_t* picks,
                                             int* hist, int hist_stride, int* hist_len, int* pos, int* left,
                                             const int* stop_mask, int* step, int64_t* const* mailbox, void* stream) {
  SP_TICK_CHECK("pdn_spec_verify_pick_tick_f32");
  PDN_CHECK_ARG(blk_max && blk_arg && n_blocks > 0, "pdn_spec_verify_pick_tick_f32: bad candidates");
  hipLaunchKernelGGL(spec_pick_kernel, dim3(B * (k + 1)), dim3(256), 0, (hipStream_t)stream, blk_max, blk_arg, n_blocks,
                     qpos, picks);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(SP_THREADS), 0, (hipStream_t)stream, tokens, qpos, picks, B, k,
                     hist, hist_stride, hist_len, pos, left, (const unsigned*)stop_mask, step, mailbox);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SPECULATE);
  return PDN_OK;
}

// PER: the pdnq_ form of include/pdn_persample.h, `params` = B blocks.
template <bool PER>
static int spec_verify_sample_tick(const float* logits, int64_t row_stride, int V, const void* params,
                                   const int64_t* tokens, const int* qpos, int B, int k, int64_t* picks, int* hist,
                                   int hist_stride, int* hist_len, int* pos, int* left, const int* stop_mask, int* step,
                                   int64_t* const* mailbox, void* stream) {
  const char* name = PER ? "pdnq_spec_verify_sample_tick_f32" : "pdn_spec_verify_sample_tick_f32";
  PDN_CHECK_ARG(tokens && qpos && picks && hist && hist_len && pos && left && step && B > 0 && k >= 0 && k <= SP_MAX_K &&
                    (int64_t)B * (k + 1) <= 65535 && hist_stride > 0,
                "%s: bad arguments (B %d, k %d, history stride %d)", name, B, k, hist_stride);
  PDN_CHECK_ARG(logits && params && V > 0 && row_stride >= V, "%s: bad logits (V %d)", name, V);
  hipLaunchKernelGGL(spec_sample_kernel<PER>, dim3(B * (k + 1)), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits,
                     row_stride, V, (const SampleParams*)params, k + 1, qpos, picks);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(SP_THREADS), 0, (hipStream_t)stream, tokens, qpos, picks, B, k,
                     hist, hist_stride, hist_len, pos, left, (const unsigned*)stop_mask, step, mailbox);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SPECULATE);
  if (PER) pdn_count(PDN_CNT_PERSAMPLE);
  return PDN_OK;
}

extern "C" int pdn_spec_verify_sample_tick_f32(const float* logits, int64_t row_stride, int V, const void* params,
                                               const int64_t* tokens, const int* qpos, int B, int k, int64_t* picks,
                                               int* hist, int hist_stride, int* hist_len, int* pos, int* left,
                                               const int* stop_mask, int* step, int64_t* const* mailbox, void* stream) {
  return spec_verify_sample_tick<false>(logits, row_stride, V, params, tokens, qpos, B, k, picks, hist, hist_stride,
                                        hist_len, pos, left, stop_mask, step, mailbox, stream);
}

extern "C" int pdnq_spec_verify_sample_tick_f32(const float* logits, int64_t row_stride, int V, const void* params,
                                                const int64_t* tokens, const int* qpos, int B, int k, int64_t* picks,
                                                int* hist, int hist_stride, int* hist_len, int* pos, int* left,
                                                const int* stop_mask, int* step, int64_t* const* mailbox, void* stream) {
  return spec_verify_sample_tick<true>(logits, row_stride, V, params, tokens, qpos, B, k, picks, hist, hist_stride,
                                       hist_len, pos, left, stop_mask, step, mailbox, stream);
}
