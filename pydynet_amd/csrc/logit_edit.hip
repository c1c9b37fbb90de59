// Per-request logit edits of a decode step (Llama.generate / generate_ragged / serve with allowed_token_ids, logit_bias,
// min_new_tokens); the contract is stated in NumPy in llm/logit_edits.py, the ABI in include/pdn_logitedit.h.  Row state,
// per plan: allow (B, ceil(V / 32)) uint32, the bits of the row's allowed set, read only where allow_on (B,) is set;
// bias_ids / bias_val (B, 1024), the row's bias table sorted by id, with bias_n (B,) entries; start (B,) int32, the position
// of the row's first generated token (its prompt length).  The step only READS the state.
//
//   logit_edit_reset_kernel  grid (4, rows listed): a listed row's bits, table, flag, count and prompt length copied from
//                            the packed sources.
//   logit_edit_kernel        grid (chunks, B): a vocabulary chunk of 1024 tokens per workgroup, 4 consecutive tokens per
//                            thread (one 16-byte load and store where the rows' addresses allow it; the 4 tokens share one
//                            word of the allowed bits and one of the stop bits).  A row's sorted bias table is staged in
//                            LDS; where its id range meets the chunk, each thread finds the place of its first token in
//                            it by binary search.  The edits in the order of the statement, then the chunk's first
//                            maximum and its index go to cand_v / cand_i (B, chunks): the layout the pick ticks reduce.
// A row at position < 0 (stopped / empty) is left untouched.
#include "common.h"

// each edit is one rounding (z + bias); nothing here may fuse
#pragma clang fp contract(off)

#define LE_THREADS 256
#define LE_PER 4
#define LE_CHUNK (LE_THREADS * LE_PER)   // 1024 tokens, 32 words of bits
#define LE_MAX_BIAS 1024                 // PDNE_MAX_BIAS of include/pdn_logitedit.h
#define LE_RESET_BLOCKS 4

struct pdne_logit_edit_params {
  int min_new_tokens;
  int reserved[3];
};

extern "C" int pdne_logit_edit_chunks(int V) { return V > 0 ? (V + LE_CHUNK - 1) / LE_CHUNK : 0; }

__global__ __launch_bounds__(LE_THREADS) void logit_edit_reset_kernel(
    unsigned* __restrict__ allow, int* __restrict__ allow_on, int* __restrict__ bias_ids, float* __restrict__ bias_val,
    int* __restrict__ bias_n, int* __restrict__ start, int B, int V, const int* __restrict__ rows,
    const unsigned* __restrict__ src_allow, const int* __restrict__ src_on, const int* __restrict__ src_ids,
    const float* __restrict__ src_val, const int* __restrict__ src_n, const int* __restrict__ src_start) {
  const int i = blockIdx.y;
  const int b = rows[i];
  if (b < 0 || b >= B) return;                   // (uniform)
  const int W = (V + 31) / 32;
  const int on = (src_allow && src_on) ? (src_on[i] != 0) : 0;
  const int n = src_n ? min(max(src_n[i], 0), LE_MAX_BIAS) : 0;
  const int t = blockIdx.x * LE_THREADS + threadIdx.x, stride = gridDim.x * LE_THREADS;
  if (on)
    for (int w = t; w < W; w += stride) allow[(int64_t)b * W + w] = src_allow[(int64_t)i * W + w];
  for (int j = t; j < n; j += stride) {
    bias_ids[(int64_t)b * LE_MAX_BIAS + j] = src_ids[(int64_t)i * LE_MAX_BIAS + j];
    bias_val[(int64_t)b * LE_MAX_BIAS + j] = src_val[(int64_t)i * LE_MAX_BIAS + j];
  }
  if (t == 0) {
    allow_on[b] = on;
    bias_n[b] = n;
    start[b] = src_start ? src_start[i] : 0;
  }
}

// the first j in [lo, hi) with ids[j] >= v (hi when there is none)
__device__ __forceinline__ int le_lower_bound(const int* ids, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// STEP: the plan's form -- g = pos - start[b] (gen_or_start = the plan's start), every pointer given (`stop` too: the
// entry passes a readable stand-in and has_stop = 0 where there is none); else g = gen_or_start[b] (null: 0) and every state
// pointer may be null.  VEC: every thread's 4 tokens are 16-byte aligned and inside the row (V % 4 == 0, row stride % 4 == 0,
// aligned base): one 16-byte load and store.
// A step is a chain of launches of a few microseconds each, so what counts here is the chain of dependent memory round
// trips, not the bytes: in the plan's form every global load -- the logits, the position, the row's flags and counts, the
// bit words, the first 256 table entries (the tables are (B, 1024) whatever the count) -- is issued straight-line, without
// a branch, before the first one is waited for (threads past V read the chunk's first tokens instead and store nothing);
// only a table of more than 256 entries costs a second trip.
template <bool STEP, bool VEC>
__global__ __launch_bounds__(LE_THREADS) void logit_edit_kernel(
    float* __restrict__ logits, int64_t rs, int V, const pdne_logit_edit_params* __restrict__ prm,
    const unsigned* __restrict__ allow, const int* __restrict__ allow_on, const int* __restrict__ bias_ids,
    const float* __restrict__ bias_val, const int* __restrict__ bias_n, const int* __restrict__ gen_or_start,
    const int* __restrict__ pos, int pos_rows, const unsigned* __restrict__ stop, int has_stop, float* __restrict__ cand_v,
    int* __restrict__ cand_i) {
  __shared__ int s_id[LE_MAX_BIAS];
  __shared__ float s_val[LE_MAX_BIAS];
  __shared__ float wv[LE_THREADS / 64];
  __shared__ int wi[LE_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = (V + 31) / 32, c0 = c * LE_CHUNK;
  float* z = logits + (int64_t)b * rs;
  const int v0 = c0 + tid * LE_PER;
  const bool in = v0 < V;
  const int vs = in ? v0 : c0;                   // (c0 < V: the grid has ceil(V / 1024) chunks)
  float x[LE_PER];
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(z + vs);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int u = 0; u < LE_PER; ++u) x[u] = z[min(vs + u, V - 1)];
  }
  const int m = prm->min_new_tokens;
  const int* gid = bias_ids + (int64_t)b * LE_MAX_BIAS;
  const float* gv = bias_val + (int64_t)b * LE_MAX_BIAS;
  int p, g0, n, id0 = 0;
  float val0 = 0.f;
  bool on;
  unsigned aw, sw;                               // (v0 % 4 == 0: a thread's 4 tokens share a word of either mask)
  if constexpr (STEP) {
    p = pos[pos_rows ? b : 0];
    g0 = gen_or_start[b];
    on = allow_on[b] != 0;
    aw = allow[(int64_t)b * W + (vs >> 5)];
    sw = stop[vs >> 5];
    n = bias_n[b];
    id0 = gid[tid];
    val0 = gv[tid];
  } else {
    p = pos ? pos[b] : 0;
    g0 = gen_or_start ? gen_or_start[b] : 0;
    on = allow && allow_on && allow_on[b];
    aw = allow ? allow[(int64_t)b * W + (vs >> 5)] : 0xffffffffu;
    sw = stop ? stop[vs >> 5] : 0u;
    n = bias_n ? bias_n[b] : 0;
    if (bias_n) {
      id0 = gid[tid];
      val0 = gv[tid];
    }
  }
  // (an empty statement that reads the loaded values: the compiler would otherwise wait for the position alone first
  //  and sink the table loads under the count, two more round trips in the chain)
  asm volatile("" ::"v"(x[0]), "v"(aw), "v"(sw), "v"(id0), "v"(val0), "s"(n), "s"(g0), "s"(m), "s"((int)on));
  if (p < 0) return;                             // (uniform) a row that computes nothing: untouched
  // the row's sorted table into LDS (uniform: n is the row's), then each thread's place in it by binary search
  n = min(max(n, 0), LE_MAX_BIAS);
  int j = 0;
  if (n > 0) {
    if (tid < n) {
      s_id[tid] = id0;
      s_val[tid] = val0;
    }
    for (int k = tid + LE_THREADS; k < n; k += LE_THREADS) {
      s_id[k] = gid[k];
      s_val[k] = gv[k];
    }
    __syncthreads();
    // (a table that ends before the chunk or begins behind it: nothing to search for)
    j = (s_id[0] >= c0 + LE_CHUNK || s_id[n - 1] < c0) ? n : le_lower_bound(s_id, 0, n, v0);
  }
  const int g = STEP ? p - g0 : g0;
  if (!on) aw = 0xffffffffu;
  if (!has_stop || g >= m) sw = 0u;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  if (in) {
#pragma unroll
    for (int u = 0; u < LE_PER; ++u) {
      const int v = v0 + u;
      if (v < V) {
        float xx = x[u];
        if (!((aw >> (v & 31)) & 1u)) xx = -INFINITY;
        if (j < n && s_id[j] == v) {
          const float bv = s_val[j];
          xx = bv == -INFINITY ? -INFINITY : xx + bv;             // (an assignment: +inf - inf would be NaN)
          ++j;
        }
        if ((sw >> (v & 31)) & 1u) xx = -INFINITY;
        x[u] = xx;
        if (xx > best || (xx == best && v < idx)) { best = xx; idx = v; }     // (ascending v: the first maximum; NaN never)
      }
    }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(z + v0) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
      for (int u = 0; u < LE_PER; ++u)
        if (v0 + u < V) z[v0 + u] = x[u];
    }
  }
  if (!cand_v) return;                           // (uniform)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { wv[wave] = best; wi[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < LE_THREADS / 64; ++w)
      if (wv[w] > best || (wv[w] == best && wi[w] < idx)) { best = wv[w]; idx = wi[w]; }
    if (idx == 0x7fffffff) {                     // nothing but NaN in the chunk: numpy.argmax's answer, its first token
      best = __int_as_float(0x7fc00000);
      idx = c0;
    }
    const int64_t o = (int64_t)b * gridDim.x + c;
    cand_v[o] = best;
    cand_i[o] = idx;
  }
}

// every group of 4 tokens of every row 16-byte aligned and whole
static bool le_vec(const float* logits, int64_t rs, int V) {
  return ((uintptr_t)logits & 15) == 0 && rs % 4 == 0 && V % 4 == 0;
}

extern "C" int pdne_logit_edit_reset(unsigned* allow, int* allow_on, int* bias_ids, float* bias_val, int* bias_n, int* start,
                                     int B, int V, const int* rows, int n_rows, const unsigned* src_allow,
                                     const int* src_allow_on, const int* src_bias_ids, const float* src_bias_val,
                                     const int* src_bias_n, const int* src_start, void* stream) {
  if (n_rows == 0) return PDN_OK;
  PDN_CHECK_ARG(allow && allow_on && bias_ids && bias_val && bias_n && start && rows && src_start && B > 0 && V > 0 &&
                    n_rows > 0 && n_rows <= 65535 && (!src_allow == !src_allow_on) &&
                    (!src_bias_ids == !src_bias_n) && (!src_bias_val == !src_bias_n),
                "pdne_logit_edit_reset: bad arguments (B %d, V %d, rows %d)", B, V, n_rows);
  hipLaunchKernelGGL(logit_edit_reset_kernel, dim3(LE_RESET_BLOCKS, n_rows), dim3(LE_THREADS), 0, (hipStream_t)stream,
                     allow, allow_on, bias_ids, bias_val, bias_n, start, B, V, rows, src_allow, src_allow_on, src_bias_ids,
                     src_bias_val, src_bias_n, src_start);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_LOGIT_EDIT);
  return PDN_OK;
}

extern "C" int pdne_logit_edit_step_f32(float* logits, int64_t row_stride, int B, int V,
                                        const pdne_logit_edit_params* params, const unsigned* allow, const int* allow_on,
                                        const int* bias_ids, const float* bias_val, const int* bias_n, const int* start,
                                        const int* pos, int pos_per_row, const unsigned* stop, float* cand_v, int* cand_i,
                                        void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && allow && allow_on && bias_ids && bias_val && bias_n && start && pos && B > 0 &&
                    B <= 65535 && V > 0 && row_stride >= V && (!cand_v == !cand_i),
                "pdne_logit_edit_step_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  // (no stop ids: the kernel still reads a word where the mask would be -- of the allowed bits -- and drops it)
  const dim3 grid(pdne_logit_edit_chunks(V), B);
  if (le_vec(logits, row_stride, V))
    hipLaunchKernelGGL((logit_edit_kernel<true, true>), grid, dim3(LE_THREADS), 0, (hipStream_t)stream, logits, row_stride,
                       V, params, allow, allow_on, bias_ids, bias_val, bias_n, start, pos, pos_per_row,
                       stop ? stop : allow, stop != nullptr, cand_v, cand_i);
  else
    hipLaunchKernelGGL((logit_edit_kernel<true, false>), grid, dim3(LE_THREADS), 0, (hipStream_t)stream, logits,
                       row_stride, V, params, allow, allow_on, bias_ids, bias_val, bias_n, start, pos, pos_per_row,
                       stop ? stop : allow, stop != nullptr, cand_v, cand_i);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_LOGIT_EDIT);
  return PDN_OK;
}

extern "C" int pdne_logit_edit_rows_f32(float* logits, int64_t row_stride, int B, int V,
                                        const pdne_logit_edit_params* params, const unsigned* allow, const int* allow_on,
                                        const int* bias_ids, const float* bias_val, const int* bias_n, const int* generated,
                                        const int* pos, const unsigned* stop, float* cand_v, int* cand_i, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && params && B > 0 && B <= 65535 && V > 0 && row_stride >= V && (!cand_v == !cand_i) &&
                    (!allow == !allow_on) && (!bias_ids == !bias_n) && (!bias_val == !bias_n),
                "pdne_logit_edit_rows_f32: bad arguments (B %d, V %d, row stride %lld)", B, V, (long long)row_stride);
  const dim3 grid(pdne_logit_edit_chunks(V), B);
  if (le_vec(logits, row_stride, V))
    hipLaunchKernelGGL((logit_edit_kernel<false, true>), grid, dim3(LE_THREADS), 0, (hipStream_t)stream, logits,
                       row_stride, V, params, allow, allow_on, bias_ids, bias_val, bias_n, generated, pos, 1, stop,
                       stop != nullptr, cand_v, cand_i);
  else
    hipLaunchKernelGGL((logit_edit_kernel<false, false>), grid, dim3(LE_THREADS), 0, (hipStream_t)stream, logits,
                       row_stride, V, params, allow, allow_on, bias_ids, bias_val, bias_n, generated, pos, 1, stop,
                       stop != nullptr, cand_v, cand_i);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_LOGIT_EDIT);
  return PDN_OK;
}
