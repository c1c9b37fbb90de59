// Token log-probabilities of a decode step or of given tokens (Llama.generate / generate_ragged / serve with
// logprobs=n, Llama.score); the contract is stated in NumPy in llm/logprobs.py: logp = float(z - lse), lse in double,
// the n best tokens by (logp desc, id asc), a row whose token is < 0 yields nan / -1 / nan.
//
// Two launches for n = 0, three for n > 0:
//   lp_stats_kernel    grid (C chunks of 2048 tokens, rows): the chunk's maximum m_c and s_c = sum exp(z - m_c) in
//                      double (per thread in index order, across lanes by the xor butterfly, across waves in wave order).
//                      Chunk 0's thread 0 reads the row's token (the tick form: from the history slot, mapped host
//                      memory: one read per row) into the workspace.
//   lp_select_kernel   grid (C, rows) for n > 0, (1, rows) for n = 0: lse = M + log(sum_c s_c * exp(m_c - M)), wave 0
//                      over the chunks in a fixed order (every workgroup of a row computes the same bits), the token's
//                      logp; n = 0: the row is written.  n > 0: the chunk's n best (logp, id) -- one wave-wide maximum
//                      per rank over 64-bit keys held in registers -- into the workspace.
//   lp_merge_kernel    n > 0, grid (rows), one wave: the chunks' lists merged, the row written.
// Ranking by logp needs lse first, hence stats before select: ranking by z within a chunk could drop a token whose logp
// rounds equal to a larger z's.  The launches order every exchange between workgroups: no fences, no atomics, and every
// sum runs in a fixed order, so two runs give the same bits.
// A key is (order-preserving bits of logp) << 32 | ~id: larger key = larger logp, then lower id; 0 = no entry (every real
// entry, -inf included, has a larger key).  The wave maximum runs on DPP row shifts plus four lane reads (no LDS).
// The standalone form reads the tokens from an array and writes three arrays.  The tick form runs after a decode tick:
// the step is (*counter - 1), the token the tick stored is read from its history slot ((*history)[slot * B + b], slot
// = step, or step % hist_ring for a ring), and row b's record of 1 + 2n int64 words (the token's logp, n ids, n logps;
// float bits zero-extended) goes to (*records)[((step % ring) * B + b) * (1 + 2n)] -- mapped host memory the host polls.
#include <climits>

#include "common.h"

#define LP_THREADS 256
#define LP_WAVES (LP_THREADS / 64)
#define LP_PER 8
#define LP_CHUNK (LP_THREADS * LP_PER)   // 2048 tokens per workgroup
#define LP_MAXN 20
#define LP_MAXCAND 4096                  // chunks * n the merging workgroup holds in LDS (64 per lane)

typedef unsigned long long lp_key;

extern "C" int pdn_logprobs_chunks(int V) { return V > 0 ? (V + LP_CHUNK - 1) / LP_CHUNK : 0; }

// workspace of R rows, C chunks, n: the rows' token logps float[R], the rows' tokens int64[R], chunk maxima float[R * C],
// chunk sums double[R * C], chunk candidates (keys) uint64[R * C * n]
struct LpWork {
  float* tlp;
  int64_t* tok;
  float* pm;
  double* ps;
  lp_key* kc;
};
static __host__ __device__ inline size_t lp_align(size_t x) { return (x + 15) & ~(size_t)15; }
static __host__ __device__ inline size_t lp_work_layout(char* base, int R, int C, int n, LpWork* w) {
  size_t o = 0;
  if (w) w->tlp = (float*)(base + o);
  o += lp_align(sizeof(float) * (size_t)R);
  if (w) w->tok = (int64_t*)(base + o);
  o += lp_align(sizeof(int64_t) * (size_t)R);
  if (w) w->pm = (float*)(base + o);
  o += lp_align(sizeof(float) * (size_t)R * C);
  if (w) w->ps = (double*)(base + o);
  o += lp_align(sizeof(double) * (size_t)R * C);
  if (w) w->kc = (lp_key*)(base + o);
  o += lp_align(sizeof(lp_key) * (size_t)R * C * n);
  return o;
}

extern "C" int64_t pdn_logprobs_work_bytes(int rows, int V, int n) {
  if (rows <= 0 || V <= 0 || n < 0) return 0;
  return (int64_t)lp_work_layout(nullptr, rows, pdn_logprobs_chunks(V), n, nullptr);
}

// where a row's token comes from: an array (standalone) or the history slot of the step a tick just finished
struct LpTok {
  const int64_t* tokens;
  int64_t* const* hist;
  const int* counter;
  int hist_ring;
};

static __device__ __forceinline__ int lp_step(const LpTok& t) { return t.counter ? *t.counter - 1 : 0; }

static __device__ __forceinline__ int64_t lp_token(const LpTok& t, int b, int B, int step) {
  if (t.tokens) return t.tokens[b];
  const int64_t slot = t.hist_ring > 0 ? step % t.hist_ring : step;
  return __hip_atomic_load(*t.hist + slot * B + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (may be host memory)
}

static __device__ __forceinline__ lp_key lp_make_key(float v, int id) {
  const unsigned u = __float_as_uint(v);
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((lp_key)k << 32) | (lp_key)(~(unsigned)id);
}
static __device__ __forceinline__ float lp_key_value(lp_key k) {
  const unsigned h = (unsigned)(k >> 32);
  return __uint_as_float((h & 0x80000000u) ? (h & 0x7fffffffu) : ~h);
}
static __device__ __forceinline__ int lp_key_id(lp_key k) { return (int)(~(unsigned)k); }

// lane i takes lane i - S of its row of 16 (0 where there is none)
template <int S>
static __device__ __forceinline__ lp_key lp_row_shr(lp_key v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, 0x110 + S, 0xf, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), 0x110 + S, 0xf, 0xf, false);
  return ((lp_key)hi << 32) | lo;
}
static __device__ __forceinline__ lp_key lp_max(lp_key a, lp_key b) { return a > b ? a : b; }
static __device__ __forceinline__ lp_key lp_lane(lp_key v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((lp_key)hi << 32) | lo;
}
// the maximum of the wave's keys, in every lane (every lane of the wave active)
static __device__ __forceinline__ lp_key lp_wave_max(lp_key v) {
  v = lp_max(v, lp_row_shr<1>(v));
  v = lp_max(v, lp_row_shr<2>(v));
  v = lp_max(v, lp_row_shr<4>(v));
  v = lp_max(v, lp_row_shr<8>(v));                         // lane 15 of each row: the row's maximum
  return lp_max(lp_max(lp_lane(v, 15), lp_lane(v, 31)), lp_max(lp_lane(v, 47), lp_lane(v, 63)));
}

__global__ __launch_bounds__(LP_THREADS) void lp_stats_kernel(const float* __restrict__ z, int64_t rs, int V, LpTok tk,
                                                              LpWork w) {
  __shared__ float wm[LP_WAVES];
  __shared__ double ws[LP_WAVES];
  const int c = blockIdx.x, b = blockIdx.y, C = gridDim.x, B = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // (one read per row: the tick form's is a host read.  Rows that yielded nothing are summed all the same: no other
  //  workgroup waits for the token)
  if (c == 0 && tid == 0) w.tok[b] = lp_token(tk, b, B, lp_step(tk));
  const float* zr = z + (int64_t)b * rs;
  const int c0 = c * LP_CHUNK;
  float x[LP_PER];
  float m = -INFINITY;
#pragma unroll
  for (int u = 0; u < LP_PER; ++u) {
    const int v = c0 + u * LP_THREADS + tid;
    x[u] = v < V ? zr[v] : -INFINITY;
    m = fmaxf(m, x[u]);
  }
  m = wave_max(m);
  if (lane == 0) wm[wave] = m;
  __syncthreads();
  m = wm[0];
  for (int k = 1; k < LP_WAVES; ++k) m = fmaxf(m, wm[k]);
  double s = 0.0;
  if (m != -INFINITY) {
#pragma unroll
    for (int u = 0; u < LP_PER; ++u)
      if (c0 + u * LP_THREADS + tid < V) s += exp((double)x[u] - (double)m);
  }
  s = wave_sum(s);
  if (lane == 0) ws[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < LP_WAVES; ++k) t += ws[k];
    w.pm[(int64_t)b * C + c] = m;
    w.ps[(int64_t)b * C + c] = t;
  }
}

// outputs of one row: the standalone arrays, or the record of the tick form
struct LpOut {
  float* tok;
  int64_t* ids;
  float* top;
  int64_t* const* rec;
  int ring;
};

static __device__ __forceinline__ void lp_put(const LpOut& o, int64_t* rrow, int b, int n, int word, int64_t id,
                                              float v) {
  // word 0: the token's logp; word 1 + r: rank r (id, logp)
  if (rrow) {
    if (word == 0) {
      __hip_atomic_store(rrow, (int64_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      __hip_atomic_store(rrow + word, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(rrow + n + word, (int64_t)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }
  if (word == 0) {
    o.tok[b] = v;
  } else {
    o.ids[(int64_t)b * n + word - 1] = id;
    o.top[(int64_t)b * n + word - 1] = v;
  }
}

__global__ __launch_bounds__(LP_THREADS) void lp_select_kernel(const float* __restrict__ z, int64_t rs, int V, int n,
                                                               int C, LpTok tk, LpWork w, LpOut o) {
  __shared__ double s_lse;
  __shared__ lp_key wl[LP_WAVES][LP_MAXN];
  const int c = blockIdx.x, b = blockIdx.y, B = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int step = lp_step(tk);
  const int64_t tok = w.tok[b];                            // (left by the stats launch: device memory)
  int64_t* rrow = o.rec ? *o.rec + ((int64_t)(step % o.ring) * B + b) * (1 + 2 * n) : nullptr;
  const float nan = __uint_as_float(0x7fc00000u);
  if (tok < 0) {                                           // (uniform) nothing yielded: nan / -1 / nan
    if (c == 0 && n == 0 && tid == 0) lp_put(o, rrow, b, n, 0, -1, nan);     // (n > 0: the merge writes the row)
    return;
  }
  if (wave == 0) {                                         // lse: wave 0 over the chunks, a fixed order
    float M = -INFINITY;
    for (int k = lane; k < C; k += 64) M = fmaxf(M, w.pm[(int64_t)b * C + k]);
    M = wave_max(M);
    double S = 0.0;
    for (int k = lane; k < C; k += 64) {
      const float mk = w.pm[(int64_t)b * C + k];
      if (mk != -INFINITY) S += w.ps[(int64_t)b * C + k] * exp((double)mk - (double)M);
    }
    S = wave_sum(S);
    if (lane == 0) s_lse = (double)M + log(S);
  }
  __syncthreads();
  const double lse = s_lse;
  const float* zr = z + (int64_t)b * rs;
  const float tok_lp = (tok < V) ? (float)((double)zr[tok] - lse) : nan;
  if (n == 0) {
    if (tid == 0) lp_put(o, rrow, b, n, 0, 0, tok_lp);
    return;
  }
  if (c == 0 && tid == 0) w.tlp[b] = tok_lp;
  // the chunk's keys in registers; rank r: the wave's maximum, its owner drops it
  const int c0 = c * LP_CHUNK;
  lp_key k[LP_PER];
#pragma unroll
  for (int u = 0; u < LP_PER; ++u) {
    const int v = c0 + u * LP_THREADS + tid;
    k[u] = v < V ? lp_make_key((float)((double)zr[v] - lse), v) : 0ull;
  }
  for (int r = 0; r < n; ++r) {
    lp_key best = 0ull;
#pragma unroll
    for (int u = 0; u < LP_PER; ++u) best = lp_max(best, k[u]);
    best = lp_wave_max(best);
#pragma unroll
    for (int u = 0; u < LP_PER; ++u)
      if (k[u] == best) k[u] = 0ull;
    if (lane == 0) wl[wave][r] = best;
  }
  __syncthreads();
  if (wave == 0) {                                         // the waves' lists (<= 80 keys): the chunk's n best
    lp_key a[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int j = lane + 64 * q;
      a[q] = j < LP_WAVES * n ? wl[j / n][j % n] : 0ull;
    }
    for (int r = 0; r < n; ++r) {
      const lp_key best = lp_wave_max(lp_max(a[0], a[1]));
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (a[q] == best) a[q] = 0ull;
      if (lane == 0) w.kc[((int64_t)b * C + c) * n + r] = best;
    }
  }
}

// grid (rows), one wave: the C lists of n keys of a row (C * n <= 4096: 64 per lane, in LDS) -> its n best
__global__ __launch_bounds__(64) void lp_merge_kernel(int n, int C, LpTok tk, LpWork w, LpOut o) {
  extern __shared__ lp_key lp_lds[];
  const int b = blockIdx.x, B = gridDim.x, lane = threadIdx.x;
  const int step = lp_step(tk);
  const int64_t tok = w.tok[b];
  int64_t* rrow = o.rec ? *o.rec + ((int64_t)(step % o.ring) * B + b) * (1 + 2 * n) : nullptr;
  const float nan = __uint_as_float(0x7fc00000u);
  if (tok < 0) {                                           // (uniform) nothing yielded: nan / -1 / nan
    for (int r = lane; r <= n; r += 64) lp_put(o, rrow, b, n, r, -1, nan);
    return;
  }
  const int total = C * n;
  for (int j = lane; j < total; j += 64) lp_lds[j] = w.kc[(int64_t)b * total + j];
  __syncthreads();
  for (int r = 0; r < n; ++r) {
    lp_key mine = 0ull;
    for (int j = lane; j < total; j += 64) mine = lp_max(mine, lp_lds[j]);
    const lp_key best = lp_wave_max(mine);
    if (best != 0ull && mine == best)                      // (keys are distinct: one owner)
      for (int j = lane; j < total; j += 64)
        if (lp_lds[j] == best) lp_lds[j] = 0ull;
    if (lane == 0)
      lp_put(o, rrow, b, n, r + 1, best ? lp_key_id(best) : -1, best ? lp_key_value(best) : nan);
  }
  if (lane == 0) lp_put(o, rrow, b, n, 0, 0, w.tlp[b]);
}

static int lp_launch(const float* logits, int64_t rs, int B, int V, int n, LpTok tk, LpOut o, void* work,
                     hipStream_t s) {
  const int C = pdn_logprobs_chunks(V);
  LpWork w;
  lp_work_layout((char*)work, B, C, n, &w);
  hipLaunchKernelGGL(lp_stats_kernel, dim3(C, B), dim3(LP_THREADS), 0, s, logits, rs, V, tk, w);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(lp_select_kernel, dim3(n > 0 ? C : 1, B), dim3(LP_THREADS), 0, s, logits, rs, V, n, C, tk, w, o);
  PDN_LAUNCH_CHECK();
  if (n > 0) {
    hipLaunchKernelGGL(lp_merge_kernel, dim3(B), dim3(64), sizeof(lp_key) * (size_t)C * n, s, n, C, tk, w, o);
    PDN_LAUNCH_CHECK();
  }
  pdn_count(PDN_CNT_LOGPROBS);
  return PDN_OK;
}

extern "C" int pdn_logprobs_rows_f32(const float* logits, int64_t row_stride, int rows, int V, int n,
                                     const int64_t* tokens, float* token_lp, int64_t* top_ids, float* top_lp, void* work,
                                     void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && tokens && token_lp && work && rows > 0 && rows <= 65535 && V > 0 && row_stride >= V &&
                    n >= 0 && n <= LP_MAXN && (n == 0 || (top_ids && top_lp)) &&
                    (int64_t)pdn_logprobs_chunks(V) * n <= LP_MAXCAND,
                "pdn_logprobs_rows_f32: bad arguments (rows %d, V %d, n %d, row stride %lld)", rows, V, n,
                (long long)row_stride);
  const LpTok tk = {tokens, nullptr, nullptr, 0};
  const LpOut o = {token_lp, top_ids, top_lp, nullptr, 1};
  return lp_launch(logits, row_stride, rows, V, n, tk, o, work, (hipStream_t)stream);
}

extern "C" int pdn_logprobs_tick_f32(const float* logits, int64_t row_stride, int B, int V, int n,
                                     int64_t* const* history, int hist_ring, const int* counter,
                                     int64_t* const* records, int ring, void* work, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && history && counter && records && work && B > 0 && B <= 65535 && V > 0 && row_stride >= V &&
                    n >= 0 && n <= LP_MAXN && ring > 0 && hist_ring >= 0 &&
                    (int64_t)pdn_logprobs_chunks(V) * n <= LP_MAXCAND,
                "pdn_logprobs_tick_f32: bad arguments (B %d, V %d, n %d, ring %d)", B, V, n, ring);
  const LpTok tk = {nullptr, history, counter, hist_ring};
  const LpOut o = {nullptr, nullptr, nullptr, records, ring};
  return lp_launch(logits, row_stride, B, V, n, tk, o, work, (hipStream_t)stream);
}
