// Chunked prefill (Llama.serve(prefill_chunk=C)): the mixed step feeds the slots' decode queries and up to C prompt
// tokens through the wide product of csrc/decode_wide.hip as one batch of query rows.  Its attention is a layout of runs,
// one per cache row r: queries q0_r .. q0_r + n_r - 1 (rows of the packed q | k | v buffer) at positions start_r ..
// start_r + n_r - 1 of cache row r.  A decode row is a run of 1; a prompt chunk is a run of up to C.
//
// Two launches, so that no workgroup reads a cache slot another workgroup of the same launch writes:
//   kv_append_rows_kernel       rotates each query's k by its position and stores k / v into the cache; a run that ends
//                               a prompt also zeroes the slot after it (the slot the first decode step attends to but
//                               never writes -- the invariant of pdn_kv_store_slots_f32).
//   extend_attention_kernel     reads only the cache: a workgroup = (run, head, key range, block of EX_QB queries); the
//                               keys of its range pass through LDS in tiles, each read once for all the block's queries,
//                               with an online softmax per query.  It leaves the key-range partials of
//                               pdn_decode_attention_rows_f32 ([m, l, 0, 0 | sum exp(s - m) v] per (query row, range,
//                               head)), which mode 3 of pdn_decode_wide_gemm_f32 merges unchanged.
// The key ranges of a run follow its last query: chunk = ceil((start + n) / NS) keys, range sp = [sp chunk, (sp + 1)
// chunk) -- for a run of 1 exactly the ranges of the decode kernel.  Every sum runs in a fixed order (no atomics).
#include "common.h"

#define EX_QB 16                 // queries per attention workgroup
#define EX_AQ 8                  // queries per append workgroup
#define EX_MAX_HD 256
#define EX_OUT (EX_QB * EX_MAX_HD / 256)    // accumulators per thread at the largest head_dim

// a run is taken only when it lies inside the query rows and the cache; anything else is skipped (never written)
__device__ __forceinline__ bool ex_run_ok(int q0, int n, int s0, int max_run, int n_q, int max_len) {
  return n > 0 && n <= max_run && q0 >= 0 && q0 + n <= n_q && s0 >= 0 && s0 + n <= max_len;
}

// grid (n_runs, ceil(max_run / EX_AQ)), 256 threads: thread = (query, interleaved pair (x[2i], x[2i+1]) of a head)
__global__ __launch_bounds__(256) void kv_append_rows_kernel(const float* __restrict__ qkv, int64_t qkv_rs,
                                                             const float* __restrict__ cs, const float* __restrict__ sn,
                                                             float* __restrict__ kc, float* __restrict__ vc, int64_t cbs,
                                                             const int* __restrict__ runs, int max_run, int n_q, int H,
                                                             int hd, int max_len) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int q0 = runs[4 * r], n = runs[4 * r + 1], s0 = runs[4 * r + 2], ends = runs[4 * r + 3];
  if (!ex_run_ok(q0, n, s0, max_run, n_q, max_len)) return;
  const int D = H * hd, half = hd / 2, pairs = D / 2;
  const int j0 = blockIdx.y * EX_AQ, j1 = min(n, j0 + EX_AQ);
  float* kb = kc + (int64_t)r * cbs;
  float* vb = vc + (int64_t)r * cbs;
  for (int e = tid; e < (j1 - j0) * pairs; e += 256) {
    const int j = j0 + e / pairs, pr = e - (e / pairs) * pairs, i = pr % half, p = s0 + j;
    const float* row = qkv + (int64_t)(q0 + j) * qkv_rs;
    const float2 k = reinterpret_cast<const float2*>(row + D)[pr];
    const float2 v = reinterpret_cast<const float2*>(row + 2 * D)[pr];
    const float c = cs[(int64_t)p * half + i], s = sn[(int64_t)p * half + i];
    reinterpret_cast<float2*>(kb + (int64_t)p * D)[pr] = make_float2(k.x * c - k.y * s, k.x * s + k.y * c);
    reinterpret_cast<float2*>(vb + (int64_t)p * D)[pr] = v;
  }
  if (ends && blockIdx.y == 0 && s0 + n < max_len) {
    const int64_t z = (int64_t)(s0 + n) * D;
    for (int d = tid; d < D; d += 256) { kb[z + d] = 0.f; vb[z + d] = 0.f; }
  }
}

// grid (n_runs * H * NS * nqb), 256 threads; dynamic LDS: q [EX_QB][hd], K tile [kt][hd + 1], V tile [kt][hd],
// probabilities [EX_QB][kt], per-query rescale factors [EX_QB]
__global__ __launch_bounds__(256) void extend_attention_kernel(const float* __restrict__ qkv, int64_t qkv_rs,
                                                               const float* __restrict__ cs, const float* __restrict__ sn,
                                                               const float* __restrict__ kc, const float* __restrict__ vc,
                                                               int64_t cbs, const int* __restrict__ runs, int max_run,
                                                               int n_q, int H, int hd, int NS, int nqb, int max_len,
                                                               float inv_sqrt, int kt, float* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float ex_lds[];
  const int tid = threadIdx.x;
  int x = blockIdx.x;
  const int qb = x % nqb; x /= nqb;
  const int sp = x % NS; x /= NS;
  const int h = x % H, r = x / H;
  const int q0 = runs[4 * r], n = runs[4 * r + 1], s0 = runs[4 * r + 2];
  if (!ex_run_ok(q0, n, s0, max_run, n_q, max_len)) return;
  const int j0 = qb * EX_QB;
  if (j0 >= n) return;
  const int nq = min(EX_QB, n - j0), D = H * hd, half = hd / 2, kp = hd + 1, rec = 4 + hd;
  const int T = s0 + n, chunk = (T + NS - 1) / NS, t0 = sp * chunk, t1 = min(T, t0 + chunk);
  const int tmax = min(t1, s0 + j0 + nq);              // (keys past the block's last query are seen by none of them)
  float* qs = ex_lds;
  float* ks = qs + EX_QB * hd;
  float* vs = ks + kt * kp;
  float* ps = vs + kt * hd;
  float* al = ps + EX_QB * kt;

  // the block's queries, rotated by their positions (queries past the run: zeros, never stored)
  for (int e = tid; e < EX_QB * half; e += 256) {
    const int q = e / half, i = e - q * half;
    float2 v = make_float2(0.f, 0.f);
    if (q < nq) {
      const int p = s0 + j0 + q;
      const float2 a = reinterpret_cast<const float2*>(qkv + (int64_t)(q0 + j0 + q) * qkv_rs + h * hd)[i];
      const float c = cs[(int64_t)p * half + i], s = sn[(int64_t)p * half + i];
      v = make_float2(a.x * c - a.y * s, a.x * s + a.y * c);
    }
    reinterpret_cast<float2*>(qs + q * hd)[i] = v;
  }

  // softmax state of query tid / 16 (16 lanes per query, identical in all 16 after each butterfly)
  const int sq = tid >> 4, sl = tid & 15;
  float m = -INFINITY, l = 0.f;
  float acc[EX_OUT];
#pragma unroll
  for (int i = 0; i < EX_OUT; ++i) acc[i] = 0.f;
  const int f4 = hd / 4, nout = EX_QB * hd;

  for (int tb = t0; tb < tmax; tb += kt) {
    const int nt = min(kt, tmax - tb);
    lds_barrier();                                     // (the previous tile's readers are done; q is staged)
    for (int e = tid; e < nt * f4; e += 256) {
      const int t = e / f4, c = e - t * f4;
      const int64_t off = (int64_t)r * cbs + (int64_t)(tb + t) * D + h * hd + 4 * c;
      const float4 k4 = *reinterpret_cast<const float4*>(kc + off);
      const float4 v4 = *reinterpret_cast<const float4*>(vc + off);
      float* kd = ks + t * kp + 4 * c;
      kd[0] = k4.x; kd[1] = k4.y; kd[2] = k4.z; kd[3] = k4.w;
      *reinterpret_cast<float4*>(vs + t * hd + 4 * c) = v4;
    }
    lds_barrier();
    // scores: thread = (query, key) pairs
    for (int e = tid; e < EX_QB * kt; e += 256) {
      const int q = e / kt, t = e - q * kt;
      float s = -INFINITY;
      if (q < nq && t < nt && tb + t < min(t1, s0 + j0 + q + 1)) {
        const float* a = qs + q * hd;
        const float* k = ks + t * kp;
        float d = 0.f;
        for (int c = 0; c < hd; c += 4) d += (a[c] * k[c] + a[c + 1] * k[c + 1]) + (a[c + 2] * k[c + 2] + a[c + 3] * k[c + 3]);
        s = d * inv_sqrt;
      }
      ps[e] = s;
    }
    lds_barrier();
    // online softmax per query: the tile's maximum, rescale, probabilities and their sum in a fixed order
    {
      float mt = -INFINITY;
      for (int t = sl; t < kt; t += 16) mt = fmaxf(mt, ps[sq * kt + t]);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) mt = fmaxf(mt, __shfl_xor(mt, o, 64));
      const float mn = fmaxf(m, mt);
      const float a = mn == -INFINITY ? 1.f : expf(m - mn);
      float ls = 0.f;
      for (int t = sl; t < kt; t += 16) {
        const float s = ps[sq * kt + t];
        const float pr = (mn == -INFINITY || s == -INFINITY) ? 0.f : expf(s - mn);
        ps[sq * kt + t] = pr;
        ls += pr;
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) ls += __shfl_xor(ls, o, 64);
      l = l * a + ls;
      m = mn;
      if (sl == 0) al[sq] = a;
    }
    lds_barrier();
    // acc = acc * rescale + P V: thread = outputs (query, column) tid, tid + 256, ...
#pragma unroll
    for (int i = 0; i < EX_OUT; ++i) {
      const int o = tid + 256 * i;
      if (o < nout) {
        const int q = o / hd, d = o - q * hd;
        float s = 0.f;
        for (int t = 0; t < nt; ++t) s = fmaf(ps[q * kt + t], vs[t * hd + d], s);
        acc[i] = acc[i] * al[q] + s;
      }
    }
  }

  // records [m, l, 0, 0 | acc] of every query of the block (no keys in this range: m = -inf, l = 0, zeros)
  if (sl == 0 && sq < nq) {
    float* out = part + (((int64_t)(q0 + j0 + sq) * NS + sp) * H + h) * rec;
    out[0] = l > 0.f ? m : -INFINITY;
    out[1] = l;
    out[2] = 0.f;
    out[3] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < EX_OUT; ++i) {
    const int o = tid + 256 * i;
    if (o < nout) {
      const int q = o / hd, d = o - q * hd;
      if (q < nq) part[(((int64_t)(q0 + j0 + q) * NS + sp) * H + h) * rec + 4 + d] = acc[i];
    }
  }
}

static int ex_kt(int hd) { return hd <= 64 ? 64 : (hd <= 128 ? 32 : 16); }

static size_t ex_lds_bytes(int hd) {
  const int kt = ex_kt(hd);
  return sizeof(float) * ((size_t)EX_QB * hd + (size_t)kt * (hd + 1) + (size_t)kt * hd + (size_t)EX_QB * kt + EX_QB);
}

extern "C" int pdn_decode_mixed_supported(int D, int H, int head_dim, int F, int V, int max_len) {
  return H > 0 && head_dim > 0 && head_dim * H == D && head_dim % 4 == 0 && head_dim <= EX_MAX_HD && D % 4 == 0 &&
         F > 0 && F % 4 == 0 && V > 0 && V <= (1 << 23) && max_len > 0 && max_len * 4 <= 60 * 1024 &&
         ex_lds_bytes(head_dim) <= 64 * 1024;
}

#define EX_CHECK(name)                                                                                                 \
  PDN_CHECK_ARG(qkv && cos_table && sin_table && k_cache && v_cache && runs && n_runs > 0 && n_runs <= 65535 &&        \
                    max_run > 0 && n_q > 0 && H > 0 && head_dim > 0 && head_dim % 4 == 0 && head_dim <= EX_MAX_HD &&    \
                    max_len > 0 && qkv_row_stride >= 3 * (int64_t)H * head_dim && qkv_row_stride % 2 == 0 &&           \
                    cache_batch_stride >= (int64_t)max_len * H * head_dim,                                            \
                name ": bad arguments (%d runs of <= %d queries, %d query rows, H %d, head_dim %d, max_len %d)",        \
                n_runs, max_run, n_q, H, head_dim, max_len);                                                           \
  PDN_CHECK_ARG(((((uintptr_t)qkv) | ((uintptr_t)k_cache) | ((uintptr_t)v_cache)) & 15) == 0 &&                        \
                    cache_batch_stride % 4 == 0,                                                                       \
                name ": 16-byte aligned q | k | v rows and caches")

extern "C" int pdn_kv_append_rows_f32(const float* qkv, int64_t qkv_row_stride, const float* cos_table,
                                      const float* sin_table, float* k_cache, float* v_cache, int64_t cache_batch_stride,
                                      const int* runs, int n_runs, int max_run, int n_q, int H, int head_dim,
                                      int max_len, void* stream) {
  if (n_runs == 0) return PDN_OK;
  EX_CHECK("pdn_kv_append_rows_f32");
  const dim3 grid(n_runs, (max_run + EX_AQ - 1) / EX_AQ);
  hipLaunchKernelGGL(kv_append_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, qkv, qkv_row_stride, cos_table,
                     sin_table, k_cache, v_cache, cache_batch_stride, runs, max_run, n_q, H, head_dim, max_len);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_EXTEND);
  return PDN_OK;
}

extern "C" int pdn_decode_extend_attention_f32(const float* qkv, int64_t qkv_row_stride, const float* cos_table,
                                               const float* sin_table, const float* k_cache, const float* v_cache,
                                               int64_t cache_batch_stride, const int* runs, int n_runs, int max_run,
                                               int n_q, int H, int head_dim, int n_splits, int max_len, float* partials,
                                               void* stream) {
  if (n_runs == 0) return PDN_OK;
  EX_CHECK("pdn_decode_extend_attention_f32");
  PDN_CHECK_ARG(partials && n_splits >= 1 && n_splits <= 64 && ex_lds_bytes(head_dim) <= 64 * 1024,
                "pdn_decode_extend_attention_f32: 1 <= n_splits <= 64 (got %d), head_dim %d", n_splits, head_dim);
  const int nqb = (max_run + EX_QB - 1) / EX_QB;
  const int64_t blocks = (int64_t)n_runs * H * n_splits * nqb;
  PDN_CHECK_ARG(blocks < ((int64_t)1 << 31), "pdn_decode_extend_attention_f32: grid too large");
  hipLaunchKernelGGL(extend_attention_kernel, dim3((unsigned)blocks), dim3(256), ex_lds_bytes(head_dim),
                     (hipStream_t)stream, qkv, qkv_row_stride, cos_table, sin_table, k_cache, v_cache,
                     cache_batch_stride, runs, max_run, n_q, H, head_dim, n_splits, nqb, max_len,
                     1.f / sqrtf((float)head_dim), ex_kt(head_dim), partials);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_EXTEND);
  return PDN_OK;
}
