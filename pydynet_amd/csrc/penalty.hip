// Repetition, presence and frequency penalties on the logits of a decode step (Llama.generate / generate_ragged / serve
// with penalties); the contract is stated in NumPy in llm/penalties.py.  Row state, per plan: counts (B, V) int32, the
// tokens each row generated, and seen (B, ceil(V / 32)) uint32, the bits of its prompt's token ids; start (B,) int32 is
// the position of its first generated token (its prompt length).
//
//   penalty_reset_kernel   grid (chunks, rows listed): zeroes the chunk's counts of a listed row and sets its prompt
//                          bits from the packed id list (each workgroup scans the prompt for the ids of ITS chunk).
//   penalty_apply_kernel   grid (chunks, B): a vocabulary chunk of 1024 tokens per workgroup.  COUNT (in the captured
//                          step): the workgroup that owns the token a row is fed counts it first, when the row is at a
//                          position past start (a generated token).  Then every token of the chunk is penalised in
//                          place and the chunk's first maximum and its index go to cand_v / cand_i (B, chunks): the
//                          layout the pick ticks reduce (largest value, lowest index among equal values).
// Each chunk has exactly one owning workgroup, so the count increment and every read of that chunk stay inside one
// workgroup -- one thread even: the thread that reads a count is the one that writes it.  No atomics, no ordering
// across workgroups.  A row at position < 0 (stopped / empty) is left untouched.
#include "common.h"

// one rounding per operation, in the order of the statement: z / r, z * r, f * c, + p, z - (...).  No FMA may form:
// the operators below are written in this file, under this pragma (the rounding helpers of the HIP headers are not,
// and two of them inlined next to each other could still be contracted); the division is the correctly rounded one.
#pragma clang fp contract(off)

#define PN_THREADS 256
#define PN_PER 4
#define PN_CHUNK (PN_THREADS * PN_PER)   // 1024 tokens, 32 words of prompt bits
#define PN_WORDS (PN_CHUNK / 32)

struct pdn_penalty_params {
  float repetition;
  float presence;
  float frequency;
  int reserved;
};

extern "C" int pdn_penalty_chunks(int V) { return V > 0 ? (V + PN_CHUNK - 1) / PN_CHUNK : 0; }

__global__ __launch_bounds__(PN_THREADS) void penalty_reset_kernel(int* __restrict__ counts, unsigned* __restrict__ seen,
                                                                   int* __restrict__ start, int B, int V,
                                                                   const int* __restrict__ rows,
                                                                   const int64_t* __restrict__ ids,
                                                                   const int* __restrict__ offsets) {
  __shared__ unsigned bits[PN_WORDS];
  const int c = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const int b = rows[i];
  if (b < 0 || b >= B) return;                   // (uniform)
  const int c0 = c * PN_CHUNK, W = (V + 31) / 32;
  int* cnt = counts + (int64_t)b * V;
#pragma unroll
  for (int u = 0; u < PN_PER; ++u) {
    const int v = c0 + u * PN_THREADS + tid;
    if (v < V) cnt[v] = 0;
  }
  if (tid < PN_WORDS) bits[tid] = 0u;
  __syncthreads();
  const int o0 = offsets[i], o1 = offsets[i + 1];
  for (int j = o0 + tid; j < o1; j += PN_THREADS) {
    const int64_t t = ids[j];
    if (t >= c0 && t < c0 + PN_CHUNK && t < V) atomicOr(&bits[(t - c0) >> 5], 1u << (t & 31));
  }
  __syncthreads();
  if (tid < PN_WORDS && c * PN_WORDS + tid < W) seen[(int64_t)b * W + c * PN_WORDS + tid] = bits[tid];
  if (c == 0 && tid == 0) start[b] = o1 - o0;
}

template <bool COUNT>
__global__ __launch_bounds__(PN_THREADS) void penalty_apply_kernel(float* __restrict__ logits, int64_t rs, int V,
                                                                   const pdn_penalty_params* __restrict__ prm,
                                                                   int* __restrict__ counts,
                                                                   const unsigned* __restrict__ seen,
                                                                   const int* __restrict__ start,
                                                                   const int64_t* __restrict__ ids,
                                                                   const int* __restrict__ pos, int pos_rows,
                                                                   float* __restrict__ cand_v, int* __restrict__ cand_i) {
  __shared__ float wv[PN_THREADS / 64];
  __shared__ int wi[PN_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p = pos ? pos[pos_rows ? b : 0] : 0;
  if (p < 0) return;                             // (uniform) a row that computes nothing: untouched
  const float r = prm->repetition, pr = prm->presence, f = prm->frequency;
  const int c0 = c * PN_CHUNK, W = (V + 31) / 32;
  float* z = logits + (int64_t)b * rs;
  int* cnt = counts ? counts + (int64_t)b * V : nullptr;
  const unsigned* sn = seen ? seen + (int64_t)b * W : nullptr;
  const int fed = (COUNT && p > start[b]) ? (int)ids[b] : -1;     // the token fed at position p - 1 >= start: generated
  float best = -INFINITY;
  int idx = 0x7fffffff;
#pragma unroll
  for (int u = 0; u < PN_PER; ++u) {
    const int v = c0 + u * PN_THREADS + tid;
    if (v < V) {
      int k = cnt ? cnt[v] : 0;
      if (COUNT && v == fed) {
        k += 1;
        cnt[v] = k;
      }
      const bool in_prompt = sn && ((sn[v >> 5] >> (v & 31)) & 1u);
      float x = z[v];
      if (in_prompt || k > 0) x = x > 0.f ? __fdiv_rn(x, r) : x * r;
      if (k > 0) x = x - (f * (float)k + pr);
      z[v] = x;
      if (x > best || (x == best && v < idx)) { best = x; idx = v; }     // (ascending v: the first maximum; NaN never)
    }
  }
  if (!cand_v) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { wv[wave] = best; wi[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PN_THREADS / 64; ++w)
      if (wv[w] > best || (wv[w] == best && wi[w] < idx)) { best = wv[w]; idx = wi[w]; }
    const int64_t o = (int64_t)b * gridDim.x + c;
    cand_v[o] = best;
    cand_i[o] = idx;
  }
}

extern "C" int pdn_penalty_reset(int* counts, unsigned* seen, int* start, int B, int V, const int* rows, int n_rows,
                                 const int64_t* ids, const int* offsets, void* stream) {
  if (n_rows == 0) return PDN_OK;
  PDN_CHECK_ARG(counts && seen && start && rows && offsets && B > 0 && V > 0 && n_rows > 0 && n_rows <= 65535,
                "pdn_penalty_reset: bad arguments (B %d, V %d, rows %d)", B, V, n_rows);
  hipLaunchKernelGGL(penalty_reset_kernel, dim3(pdn_penalty_chunks(V), n_rows), dim3(PN_THREADS), 0,
                     (hipStream_t)stream, counts, seen, start, B, V, rows, ids, offsets);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_PENALTY);
  return PDN_OK;
}

extern "C" int pdn_penalty_step_f32(float* logits, int64_t row_stride, int B, int V, const pdn_penalty_params* params,
                                    int* counts, const unsigned* seen, const int* start, const int64_t* ids,
                                    const int* pos, int pos_per_row, float* cand_v, int* cand_i, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && counts && seen && start && ids && pos && B > 0 && B <= 65535 && V > 0 &&
                    row_stride >= V && (!cand_v == !cand_i),
                "pdn_penalty_step_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  hipLaunchKernelGGL(penalty_apply_kernel<true>, dim3(pdn_penalty_chunks(V), B), dim3(PN_THREADS), 0,
                     (hipStream_t)stream, logits, row_stride, V, params, counts, seen, start, ids, pos, pos_per_row,
                     cand_v, cand_i);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_PENALTY);
  return PDN_OK;
}

extern "C" int pdn_penalty_rows_f32(float* logits, int64_t row_stride, int B, int V, const pdn_penalty_params* params,
                                    const int* counts, const unsigned* seen, const int* pos, float* cand_v, int* cand_i,
                                    void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && B > 0 && B <= 65535 && V > 0 && row_stride >= V && (!cand_v == !cand_i),
                "pdn_penalty_rows_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  hipLaunchKernelGGL(penalty_apply_kernel<false>, dim3(pdn_penalty_chunks(V), B), dim3(PN_THREADS), 0,
                     (hipStream_t)stream, logits, row_stride, V, params, const_cast<int*>(counts), seen, nullptr,
                     nullptr, pos, 1, cand_v, cand_i);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_PENALTY);
  return PDN_OK;
}
