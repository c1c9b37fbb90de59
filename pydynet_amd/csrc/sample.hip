// Sampled next token: temperature, top-k and top-p (nucleus) over full fp32 logit rows -- the generalisation of the
// greedy pick of llm/llama/model.py:258-269 (argmax(-1)) that `Llama.generate(..., temperature > 0)` runs.
//
// Contract (pydynet_amd/llm/sampling.py states it in NumPy; include/pdn_hip.h): for one row z of V logits and
// temperature T > 0
//   1. top-k: keep every token with z_i >= z_(k), the k-th largest value counting repeats (k = 0 or k >= V: off);
//   2. p_i = exp((z_i - max z) / T) over the kept tokens, normalised;
//   3. top-p: theta = the largest kept value whose mass of {kept i : z_i >= theta} is at least top_p; keep those
//      (top_p >= 1: off);
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
#include <stddef.h>

#include "common.h"

// include/pdn_hip.h: pdn_sample_params (the header is C and is not included by the kernels)
struct SampleParams {
  float temperature;
  int top_k;
  float top_p;
  uint64_t seed;
};
static_assert(sizeof(SampleParams) == 24 && offsetof(SampleParams, seed) == 16, "pdn_sample_params layout");

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)
#define SMP_BINS 4096

struct SmpShared {
  unsigned long long hist[SMP_BINS];
  unsigned long long wtot[SMP_WAVES];
  float fmax[SMP_WAVES];
  int farg[SMP_WAVES];
  unsigned sel;
  unsigned long long sel_above;
  int tok;
};

// order-preserving: a < b (as floats, no NaN) <=> key(a) < key(b)
__device__ __forceinline__ unsigned smp_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Philox4x64-10 (Salmon et al., SC'11), first word of the block for counter (c0, c1, 0, 0) and key (k0, 0)
__device__ __forceinline__ uint64_t smp_philox_w0(uint64_t c0, uint64_t c1, uint64_t k0) {
  uint64_t c2 = 0, c3 = 0, k1 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
    const uint64_t hi0 = __umul64hi(0xD2E7470EE14C6C93ull, c0), lo0 = 0xD2E7470EE14C6C93ull * c0;
    const uint64_t hi1 = __umul64hi(0xCA5A826395121157ull, c2), lo1 = 0xCA5A826395121157ull * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
  }
  return c0;
}

// integer weight of a logit: exp((z - m) / T) in [0, 1] scaled by 2^40 (NaN -> 0)
__device__ __forceinline__ unsigned long long smp_weight(float z, float m, float T) {
  const float e = expf((z - m) / T);
  return e >= 0.f ? (unsigned long long)(e * 1099511627776.f) : 0ull;
}

// inclusive scan of one value per thread over the workgroup (in thread order); *total = the sum of all
__device__ __forceinline__ unsigned long long smp_scan(unsigned long long v, SmpShared& s, unsigned long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  if (lane == 63) s.wtot[wave] = v;
  __syncthreads();
  unsigned long long off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) {
    const unsigned long long x = s.wtot[w];
    off += w < wave ? x : 0ull;
    tot += x;
  }
  __syncthreads();                                   // (wtot is rewritten by the next scan)
  *total = tot;
  return v + off;
}

// The largest key K such that the weight of {i : key_i >= K, key_i >= floor} is at least `need` (MASS: weights w_i and
// need = ceil(p * total weight above floor); else counts and need = k).  Levels of 12, 12 and 8 key bits.
template <bool MASS>
__device__ __forceinline__ unsigned smp_select(const float* __restrict__ row, int V, unsigned floor, float m, float T,
                                               float p, unsigned long long need, SmpShared& s) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, pmask = 0;
  unsigned long long above = 0;                      // weight of the keys above the current prefix's range
#pragma unroll 1
  for (int lv = 0; lv < 3; ++lv) {
    const int sh = lv == 0 ? 20 : lv == 1 ? 8 : 0;
    const unsigned nb = lv == 2 ? 256u : 4096u;
    for (int i = tid; i < SMP_BINS; i += SMP_THREADS) s.hist[i] = 0;
    if (tid == 0) { s.sel = 0; s.sel_above = above; }     // (only a row with NaNs can leave these in place)
    __syncthreads();
    for (int i = tid; i < V; i += SMP_THREADS) {
      const float z = row[i];
      const unsigned k = smp_key(z);
      if (k >= floor && (k & pmask) == prefix) {
        const unsigned long long w = MASS ? smp_weight(z, m, T) : 1ull;
        if (w) atomicAdd(&s.hist[(k >> sh) & (nb - 1)], w);      // integer: the sum does not depend on the order
      }
    }
    __syncthreads();
    // thread t owns bins nb-1-4t .. nb-4-4t: a scan in thread order is a suffix sum over the bins
    unsigned long long h[4], part = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int bin = (int)nb - 1 - 4 * tid - q;
      h[q] = bin >= 0 ? s.hist[bin] : 0ull;
      part += h[q];
    }
    unsigned long long tot;
    const unsigned long long incl = smp_scan(part, s, &tot);
    if (MASS && lv == 0) {
      // tot = the mass of every token above the floor (the kept set of step 1)
      const double want = ceil((double)p * (double)tot);
      need = want < 1.0 ? 1ull : want >= (double)tot ? tot : (unsigned long long)want;
    }
    unsigned long long run = above + incl - part;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int bin = (int)nb - 1 - 4 * tid - q;
      if (bin >= 0 && run < need && run + h[q] >= need) { s.sel = (unsigned)bin; s.sel_above = run; }
      run += h[q];
    }
    __syncthreads();
    prefix |= s.sel << sh;
    pmask |= (nb - 1) << sh;
    above = s.sel_above;
    __syncthreads();                                 // (sel is rewritten by the next level)
  }
  return prefix;
}

// the sampled token of one row (every thread of the workgroup calls it and gets the token)
__device__ __forceinline__ int smp_row(const float* __restrict__ row, int V, const SampleParams prm, uint64_t t,
                                       uint64_t b, SmpShared& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // max and its first index
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  for (int i = tid; i < V; i += SMP_THREADS) {
    const float z = row[i];
    if (z > mx) { mx = z; arg = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(arg, o, 64);
    if (ov > mx || (ov == mx && oi < arg)) { mx = ov; arg = oi; }
  }
  if (lane == 0) { s.fmax[wave] = mx; s.farg[wave] = arg; }
  __syncthreads();
  mx = s.fmax[0]; arg = s.farg[0];
#pragma unroll
  for (int w = 1; w < SMP_WAVES; ++w)
    if (s.fmax[w] > mx || (s.fmax[w] == mx && s.farg[w] < arg)) { mx = s.fmax[w]; arg = s.farg[w]; }
  if (arg == 0x7fffffff) arg = 0;                    // (a row of NaNs: token 0, as numpy.argmax)
  const float T = prm.temperature;
  if (!(T > 0.f)) return arg;                         // (the host never asks: T = 0 is the greedy path)

  unsigned floor = 0;
  if (prm.top_k > 0 && prm.top_k < V) floor = smp_select<false>(row, V, 0u, mx, T, 1.f, (unsigned long long)prm.top_k, s);
  if (prm.top_p < 1.f) floor = smp_select<true>(row, V, floor, mx, T, prm.top_p, 0ull, s);

  // draw: chunk sums, block scan, the chunk holding the target is walked by its thread
  const int C = (V + SMP_THREADS - 1) / SMP_THREADS;
  const int lo = min(tid * C, V), hi = min(lo + C, V);
  unsigned long long part = 0;
  for (int i = lo; i < hi; ++i) {
    const float z = row[i];
    if (smp_key(z) >= floor) part += smp_weight(z, mx, T);
  }
  if (tid == 0) s.tok = arg;                         // (kept mass 0: only with NaNs)
  unsigned long long W;
  const unsigned long long incl = smp_scan(part, s, &W);
  // u * W with u = r * 2^-24: the token is the first whose inclusive prefix exceeds floor(r * W / 2^24)
  const unsigned long long r = smp_philox_w0(t, b, prm.seed) >> 40;
  const unsigned long long target = r * (W >> 24) + ((r * (W & 0xFFFFFFull)) >> 24);
  const unsigned long long excl = incl - part;
  if (W > 0 && excl <= target && target < incl) {
    unsigned long long run = excl;
    for (int i = lo; i < hi; ++i) {
      const float z = row[i];
      if (smp_key(z) >= floor) {
        run += smp_weight(z, mx, T);
        if (run > target) { s.tok = i; break; }
      }
    }
  }
  __syncthreads();
  return s.tok;
}

__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(const float* __restrict__ logits, int64_t rs, int V,
                                                                 const SampleParams* __restrict__ prm, int64_t t,
                                                                 int64_t* __restrict__ out) {
  __shared__ SmpShared s;
  const int b = blockIdx.x;
  const int tok = smp_row(logits + (int64_t)b * rs, V, *prm, (uint64_t)t, (uint64_t)b, s);
  if (threadIdx.x == 0) out[b] = tok;
}

extern "C" int pdn_sample_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params, int64_t t,
                                   int64_t* out_ids, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && out_ids && B > 0 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "pdn_sample_rows_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  PDN_CHECK_ARG(t >= 0, "pdn_sample_rows_f32: negative counter %lld", (long long)t);
  hipLaunchKernelGGL(sample_rows_kernel, dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                     (const SampleParams*)params, t, out_ids);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
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
template <bool ROWS, bool SLOTS = false>
__global__ __launch_bounds__(SMP_THREADS) void decode_sample_tick_kernel(
    const float* __restrict__ logits, int64_t rs, int B, int V, const SampleParams* __restrict__ prm,
    int64_t* __restrict__ ids, int* __restrict__ pos, int64_t* const* __restrict__ hist, const float* __restrict__ emb,
    int64_t emb_rs, int D, float* __restrict__ x_next, int* __restrict__ step, const unsigned* __restrict__ stop,
    const int* __restrict__ req, int* __restrict__ left, int ring) {
  __shared__ SmpShared s;
  const int tid = threadIdx.x;
  const int p = ROWS ? *step : (pos ? *pos : 0);
  const SampleParams pr = *prm;
  int64_t* hrow = hist ? *hist + (int64_t)(SLOTS ? p % ring : p) * B : nullptr;
  for (int b = 0; b < B; ++b) {
    const int pb = ROWS ? pos[b] : p;      // (read by every thread before the barriers of smp_row)
    if (ROWS && pb < 0) {                  // (uniform)
      if (tid == 0 && hrow) __hip_atomic_store(hrow + b, (int64_t)-1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      continue;
    }
    const int64_t tok = smp_row(logits + (int64_t)b * rs, V, pr, (uint64_t)pb, (uint64_t)(SLOTS ? req[b] : b), s);
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
extern "C" int pdn_decode_sample_tick_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                               int64_t* next_ids, int* pos, int* step, const unsigned* stop_mask,
                                               int64_t* const* history, const float* emb, int64_t emb_row_stride, int D,
                                               float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && next_ids && pos && step && B > 0 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "pdn_decode_sample_tick_rows_f32: bad arguments (B %d, V %d)", B, V);
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "pdn_decode_sample_tick_rows_f32: an embedding table needs x_next and D");
  hipLaunchKernelGGL(decode_sample_tick_kernel<true>, dim3(1), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits,
                     row_stride, B, V, (const SampleParams*)params, next_ids, pos, history, emb, emb_row_stride, D, x_next,
                     step, stop_mask, nullptr, nullptr, 0);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_DECODE_ROWS);
  return PDN_OK;
}

// The per-row tick of a served batch (decode_sample_tick_kernel<true, true>): as pdn_decode_sample_tick_rows_f32, but
// row b is drawn with counter (pos[b], req[b]), left (B,) int32 counts the tokens row b may still produce and the
// history is a ring of `ring` steps, (*history)[(*step % ring) * B + b].
extern "C" int pdn_decode_sample_tick_slots_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                                int64_t* next_ids, int* pos, int* step, const int* req, int* left,
                                                int ring, const unsigned* stop_mask, int64_t* const* history,
                                                const float* emb, int64_t emb_row_stride, int D, float* x_next,
                                                void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && next_ids && pos && step && req && left && ring > 0 && B > 0 && V > 0 &&
                    V <= (1 << 23) && row_stride >= V,
                "pdn_decode_sample_tick_slots_f32: bad arguments (B %d, V %d, ring %d)", B, V, ring);
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "pdn_decode_sample_tick_slots_f32: an embedding table needs x_next and D");
  hipLaunchKernelGGL((decode_sample_tick_kernel<true, true>), dim3(1), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits,
                     row_stride, B, V, (const SampleParams*)params, next_ids, pos, history, emb, emb_row_stride, D, x_next,
                     step, stop_mask, req, left, ring);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_DECODE_SLOTS);
  return PDN_OK;
}
