// Beam search in the graph-replayed decode step (Llama.beam_search; the contract is stated in NumPy in
// pydynet_amd/llm/beam.py).  After a step's vocabulary projection has written full logit rows:
//   beam_topk_kernel     one workgroup per live row: log-sum-exp, the W best non-stop tokens (logp, id), every stop
//                        id's logp;
//   beam_select_kernel   one workgroup per group of W beam rows: merges their candidates, writes the next beams, the
//                        finished hypotheses and the history; the last group to arrive publishes the live-group count;
//   kv_reorder_kernel    every row's KV history becomes its parent row's, in place.
// No float atomics anywhere; every sum runs in a fixed order, so two runs give the same bits.
#include <algorithm>

#include "common.h"

#define BM_THREADS 512
#define BM_WAVES (BM_THREADS / 64)
#define BM_MAXW 16
#define BM_MAXS 16
#define BM_LDS_KEYS 36864                    // rows up to this many tokens sit in LDS as keys (144 KiB)
#define BM_MAX_V (1 << 20)                   // global path: the stop bitmask of V tokens in LDS (128 KiB)

// order-preserving: a < b (as floats, no NaN) <=> key(a) < key(b); 0 marks an excluded token
__device__ __forceinline__ unsigned bm_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bm_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long bm_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// grid (B), BM_THREADS threads; dynamic LDS: V keys (LDS) or ceil(V / 32) stop-mask words (GLOBAL).
// Row r (skipped when pos[r] < 0; with `first`, only rows r % W == 0, which read logit row r / W): m = max z,
// lse = m + log(sum exp(z - m)) in double, summed per thread in index order and across threads in thread order.
// The W best non-stop tokens by (z desc, id asc) -> cand_lp / cand_id (r, W), logp = float(z - lse); stop j's logp ->
// stop_lp (r, n_stops).  Round k takes the largest packed (key << 32 | ~id) below round k - 1's: no token is marked.
template <bool LDS>
__global__ __launch_bounds__(BM_THREADS) void beam_topk_kernel(const float* __restrict__ logits, int64_t rs, int V, int W,
                                                               int first, const int* __restrict__ pos,
                                                               const int* __restrict__ stops, int n_stops,
                                                               float* __restrict__ cand_lp, int* __restrict__ cand_id,
                                                               float* __restrict__ stop_lp) {
  extern __shared__ __attribute__((aligned(16))) unsigned bm_lds[];
  __shared__ unsigned long long red[2][BM_WAVES];
  __shared__ double dsum[BM_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((pos && pos[r] < 0) || (first && r % W)) return;
  const float* z = logits + (int64_t)(first ? r / W : r) * rs;
  // pass 1: keys (staged in LDS) and the row maximum
  unsigned kmax = 0;
  if (!LDS)
    for (int i = tid; i < (V + 31) / 32; i += BM_THREADS) bm_lds[i] = 0u;
  for (int i = tid; i < V; i += BM_THREADS) {
    const unsigned k = bm_key(z[i]);
    if (LDS) bm_lds[i] = k;
    kmax = k > kmax ? k : kmax;
  }
  unsigned long long mv = bm_wave_max((unsigned long long)kmax);
  if (lane == 0) red[0][wave] = mv;
  __syncthreads();
  if (!LDS && tid < n_stops && stops[tid] >= 0 && stops[tid] < V)
    atomicOr(&bm_lds[stops[tid] >> 5], 1u << (stops[tid] & 31));   // (integer: order-free)
  mv = 0;
  for (int w = 0; w < BM_WAVES; ++w) mv = red[0][w] > mv ? red[0][w] : mv;
  const float m = bm_unkey((unsigned)mv);
  // pass 2: sum of exp(z - m), double
  double s = 0.0;
  for (int i = tid; i < V; i += BM_THREADS) s += exp((double)(LDS ? bm_unkey(bm_lds[i]) : z[i]) - (double)m);
  s = wave_sum(s);
  if (lane == 0) dsum[wave] = s;
  __syncthreads();
  double tot = 0.0;
  for (int w = 0; w < BM_WAVES; ++w) tot += dsum[w];
  const double lse = (double)m + log(tot);
  if (tid < n_stops) {
    const int t = min(max(stops[tid], 0), V - 1);             // (in range by contract; clamped all the same)
    stop_lp[(int64_t)r * n_stops + tid] = (float)((double)z[t] - lse);
    if (LDS && t == stops[tid]) bm_lds[t] = 0u;                // (the LDS path excludes stops by key 0)
  }
  __syncthreads();
  // W rounds of a block-wide max over the packed candidates below the previous round's
  unsigned long long prev = ~0ull;
  for (int k = 0; k < W; ++k) {
    unsigned long long best = 0;
    for (int i = tid; i < V; i += BM_THREADS) {
      unsigned key;
      if (LDS) {
        key = bm_lds[i];
      } else {
        key = ((bm_lds[i >> 5] >> (i & 31)) & 1u) ? 0u : bm_key(z[i]);
      }
      const unsigned long long p = ((unsigned long long)key << 32) | (unsigned)(0xffffffffu - (unsigned)i);
      if (key && p < prev && p > best) best = p;
    }
    best = bm_wave_max(best);
    if (lane == 0) red[k & 1][wave] = best;
    __syncthreads();
    best = 0;
    for (int w = 0; w < BM_WAVES; ++w) best = red[k & 1][w] > best ? red[k & 1][w] : best;
    prev = best;
    if (tid == 0) {
      const int id = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
      cand_id[(int64_t)r * W + k] = best ? id : -1;
      cand_lp[(int64_t)r * W + k] = best ? (float)((double)bm_unkey((unsigned)(best >> 32)) - lse) : -INFINITY;
    }
  }
}

extern "C" int pdn_beam_topk_rows_f32(const float* logits, int64_t row_stride, int B, int V, int W, int first,
                                      const int* pos, const int* stops, int n_stops, float* cand_lp, int* cand_id,
                                      float* stop_lp, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && cand_lp && cand_id && B > 0 && V > 0 && V <= BM_MAX_V && row_stride >= V && W >= 1 &&
                    W <= BM_MAXW && n_stops >= 0 && n_stops <= BM_MAXS && V - n_stops >= W &&
                    (n_stops == 0 || (stops && stop_lp)) && (!first || B % W == 0),
                "pdn_beam_topk_rows_f32: bad arguments (B %d, V %d, W %d, %d stops)", B, V, W, n_stops);
  static bool attr = false;
  if (!attr) {
    PDN_HIP(hipFuncSetAttribute((const void*)beam_topk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                BM_LDS_KEYS * 4));
    PDN_HIP(hipFuncSetAttribute((const void*)beam_topk_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                BM_MAX_V / 8));
    attr = true;
  }
  if (V <= BM_LDS_KEYS)
    hipLaunchKernelGGL(beam_topk_kernel<true>, dim3(B), dim3(BM_THREADS), (size_t)V * 4, (hipStream_t)stream, logits,
                       row_stride, V, W, first, pos, stops, n_stops, cand_lp, cand_id, stop_lp);
  else
    hipLaunchKernelGGL(beam_topk_kernel<false>, dim3(B), dim3(BM_THREADS), (size_t)(V + 31) / 32 * 4,
                       (hipStream_t)stream, logits, row_stride, V, W, first, pos, stops, n_stops, cand_lp, cand_id,
                       stop_lp);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_BEAM);
  return PDN_OK;
}

// grid (G), 256 threads.  Group g holds rows g * W + j.  Skipped (it only counts in) when pos[g * W] < 0: done.
// Candidates: beam j < (first ? 1 : W), its W non-stop tokens and its n_stops stop ids, score float(scores[r] +
// logp) (first: score 0).  Ordered by (score desc, beam asc, token asc): a candidate's rank = how many candidates beat
// it, counted over all (rank_all) and over the non-stop ones (rank_ns).  Non-stop with rank_ns < W: next beam rank_ns.
// Stop with rank_all < W: a finished entry (step, parent beam, stop id, raw score), appended in rank order.
#define SEL_THREADS 256
#define SEL_MAXC (2 * BM_MAXW * BM_MAXW)
__global__ __launch_bounds__(SEL_THREADS) void beam_select_kernel(
    const float* __restrict__ cand_lp, const int* __restrict__ cand_id, const float* __restrict__ stop_lp,
    const int* __restrict__ stops, int n_stops, int G, int W, int first, float* __restrict__ scores,
    int64_t* __restrict__ next_ids, int* __restrict__ parent, int* __restrict__ pos, int* step, int* arrive,
    int* live_acc, int* __restrict__ hist, int n_hist, int* __restrict__ fin_n, int* __restrict__ fin,
    int64_t* live_out, int n_live, const float* __restrict__ emb, int64_t emb_rs, int D, float* __restrict__ x_next) {
  __shared__ float sc[SEL_MAXC];
  __shared__ int bt[SEL_MAXC], tk[SEL_MAXC];    // beam, token
  __shared__ int nb_tok[BM_MAXW], nb_par[BM_MAXW], fs[BM_MAXW];
  __shared__ float nb_sc[BM_MAXW];
  __shared__ int s_done, s_step;
  const int g = blockIdx.x, tid = threadIdx.x, B = G * W, r0 = g * W;
  if (tid == 0) s_step = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int p0 = pos[r0];
  if (p0 >= 0) {
    const int nb = first ? 1 : W, nns = nb * W, nc = nns + nb * n_stops;
    for (int c = tid; c < nc; c += SEL_THREADS) {
      int b, t;
      float lp;
      if (c < nns) {
        b = c / W;
        lp = cand_lp[(int64_t)(r0 + b) * W + c % W];
        t = cand_id[(int64_t)(r0 + b) * W + c % W];
      } else {
        b = (c - nns) / n_stops;
        lp = stop_lp[(int64_t)(r0 + b) * n_stops + (c - nns) % n_stops];
        t = stops[(c - nns) % n_stops];
      }
      sc[c] = (first ? 0.f : scores[r0 + b]) + lp;
      bt[c] = b;
      tk[c] = t;
    }
    if (tid < BM_MAXW) fs[tid] = -1;
    __syncthreads();
    for (int c = tid; c < nc; c += SEL_THREADS) {
      const float s = sc[c];
      const int b = bt[c], t = tk[c];
      int rank_all = 0, rank_ns = 0;
      for (int o = 0; o < nc; ++o) {
        const float so = sc[o];
        const bool beats = so > s || (so == s && (bt[o] < b || (bt[o] == b && tk[o] < t)));
        rank_all += beats;
        rank_ns += beats && o < nns;
      }
      if (c < nns && rank_ns < W) {
        nb_tok[rank_ns] = t;
        nb_par[rank_ns] = b;
        nb_sc[rank_ns] = s;
      } else if (c >= nns && rank_all < W) {
        fs[rank_all] = c;
      }
    }
    __syncthreads();
    const int sp = s_step;
    if (tid == 0) {
      int n = fin_n[g];
      for (int k = 0; k < W; ++k) {
        const int c = fs[k];
        if (c < 0 || n >= 2 * W - 1) continue;
        int* e = fin + ((int64_t)g * (2 * W - 1) + n) * 4;
        e[0] = sp;
        e[1] = bt[c];
        e[2] = tk[c];
        e[3] = __float_as_int(sc[c]);
        ++n;
      }
      fin_n[g] = n;
      s_done = n >= W;
    }
    __syncthreads();
    const bool done = s_done;
    if (tid < W) {
      const int r = r0 + tid;
      if (sp < n_hist) {
        hist[((int64_t)sp * B + r) * 2] = nb_tok[tid];
        hist[((int64_t)sp * B + r) * 2 + 1] = nb_par[tid];
      }
      scores[r] = nb_sc[tid];
      next_ids[r] = nb_tok[tid];
      parent[r] = done ? r : r0 + nb_par[tid];
      pos[r] = done ? -1 : p0 + 1;
    }
    if (x_next && !done)
      for (int e = tid; e < W * D; e += SEL_THREADS) {
        const int j = e / D;
        x_next[(int64_t)(r0 + j) * D + e % D] = emb[(int64_t)max(nb_tok[j], 0) * emb_rs + e % D];
      }
    if (tid == 0 && !done) __hip_atomic_fetch_add(live_acc, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // count in (after every read of *step): the last group publishes the live count and advances the step
  __syncthreads();
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (old == G - 1) {
      const int n = __hip_atomic_load(live_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(live_acc, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(step, s_step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (live_out && s_step < n_live)       // (may be host memory)
        __hip_atomic_store(live_out + s_step, (int64_t)n, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

extern "C" int pdn_beam_select_f32(const float* cand_lp, const int* cand_id, const float* stop_lp, const int* stops,
                                   int n_stops, int G, int W, int first, float* scores, int64_t* next_ids, int* parent,
                                   int* pos, int* step, int* arrive, int* live_acc, int* hist, int n_hist, int* fin_n,
                                   int* fin, int64_t* live_out, int n_live, const float* emb, int64_t emb_row_stride,
                                   int D, float* x_next, void* stream) {
  if (G == 0) return PDN_OK;
  PDN_CHECK_ARG(cand_lp && cand_id && scores && next_ids && parent && pos && step && arrive && live_acc && fin_n && fin &&
                    G > 0 && W >= 1 && W <= BM_MAXW && (int64_t)G * W <= 65536 && n_stops >= 0 &&
                    n_stops <= BM_MAXS && (n_stops == 0 || (stops && stop_lp)) && n_hist >= 0 && (!hist || n_hist) &&
                    n_live >= 0 && (!x_next || (emb && D > 0 && emb_row_stride >= D)),
                "pdn_beam_select_f32: bad arguments (%d groups of %d, %d stops, D %d)", G, W, n_stops, D);
  hipLaunchKernelGGL(beam_select_kernel, dim3(G), dim3(SEL_THREADS), 0, (hipStream_t)stream, cand_lp, cand_id, stop_lp,
                     stops, n_stops, G, W, first, scores, next_ids, parent, pos, step, arrive, live_acc, hist,
                     hist ? n_hist : 0, fin_n, fin, live_out, n_live, emb, emb_row_stride, D, x_next);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_BEAM);
  return PDN_OK;
}

// grid (ceil(D / 4 / KVR_C4), PY, n_tensors), 256 threads.  Row r moves when parent[r] != r and pos[r] > 0: positions
// [0, min(pos[r], max_len)) of row parent[r] become row r's.  A workgroup owns (tensor, column slice) at positions
// t = blockIdx.y + k * PY, for ALL rows: it loads every moving row's source there, waits, then stores -- no other
// workgroup touches those bytes, so the gather is in place and race-free.
#define KVR_C4 8                   // float4 columns per slice
#define KVR_ROWS 256
__global__ __launch_bounds__(256) void kv_reorder_kernel(float* const* __restrict__ caches, int64_t bs, int B, int D,
                                                         const int* __restrict__ parent, const int* __restrict__ pos,
                                                         int max_len) {
  __shared__ int s_par[KVR_ROWS], s_n[KVR_ROWS];
  __shared__ int s_tmax[4];
  const int tid = threadIdx.x;
  int n = 0;
  if (tid < B) {
    const int p = parent[tid], q = pos[tid];
    n = (p != tid && p >= 0 && p < B && q > 0) ? min(q, max_len) : 0;
    s_par[tid] = p;
    s_n[tid] = n;
  }
  int m = n;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) s_tmax[tid >> 6] = m;
  __syncthreads();
  const int tmax = max(max(s_tmax[0], s_tmax[1]), max(s_tmax[2], s_tmax[3]));
  float* base = caches[blockIdx.z];
  const int D4 = D / 4, c0 = blockIdx.x * KVR_C4, cw = min(KVR_C4, D4 - c0);
  for (int t = blockIdx.y; t < tmax; t += gridDim.y) {
    // thread tid handles column c = tid % KVR_C4 of rows tid / KVR_C4 + 32 k
    const int c = tid % KVR_C4, rb = tid / KVR_C4;
    float4 v[KVR_ROWS * KVR_C4 / 256];
#pragma unroll
    for (int k = 0; k < KVR_ROWS * KVR_C4 / 256; ++k) {
      const int r = rb + k * (256 / KVR_C4);
      v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r < B && c < cw && t < s_n[r])
        v[k] = *reinterpret_cast<const float4*>(base + (int64_t)s_par[r] * bs + (int64_t)t * D + 4 * (c0 + c));
    }
    __syncthreads();                              // (every source of position t is loaded before any store)
#pragma unroll
    for (int k = 0; k < KVR_ROWS * KVR_C4 / 256; ++k) {
      const int r = rb + k * (256 / KVR_C4);
      if (r < B && c < cw && t < s_n[r])
        *reinterpret_cast<float4*>(base + (int64_t)r * bs + (int64_t)t * D + 4 * (c0 + c)) = v[k];
    }
  }
}

extern "C" int pdn_kv_reorder_rows_f32(float* const* caches, int n_tensors, int64_t batch_stride, int B, int max_len,
                                       int D, const int* parent, const int* pos, void* stream) {
  if (n_tensors == 0 || B == 0) return PDN_OK;
  PDN_CHECK_ARG(caches && parent && pos && n_tensors > 0 && n_tensors <= 65535 && B > 0 && B <= KVR_ROWS &&
                    max_len > 0 && D > 0 && D % 4 == 0 && batch_stride >= (int64_t)max_len * D && batch_stride % 4 == 0,
                "pdn_kv_reorder_rows_f32: bad arguments (%d tensors, B %d, length %d, D %d)", n_tensors, B, max_len, D);
  const int slices = (D / 4 + KVR_C4 - 1) / KVR_C4;
  const int py = (int)std::max<int64_t>(1, std::min<int64_t>(max_len, cdiv64(4096, (int64_t)slices * n_tensors)));
  hipLaunchKernelGGL(kv_reorder_kernel, dim3(slices, py, n_tensors), dim3(256), 0, (hipStream_t)stream, caches,
                     batch_stride, B, D, parent, pos, max_len);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_BEAM);
  return PDN_OK;
}
