// Decode attention of a sliding-window model for gfx950: the statement of pdnj_decode_attention_f32 (decode_gqa.hip) with
// the keys [lo, pos], lo = max(0, pos - window + 1), instead of [0, pos] -- RoPE of the new q / k rows, KV-cache append to
// the LINEAR cache row pos, attention of the one new query per head over the last `window` keys.  G = H / Hkv from 1 to 8:
// a windowed multi-head model (G = 1) and a windowed grouped model share this kernel.  include/pdn_banddecode.h (prefix
// pdnv_); statement: tests/abi_emulator/_banddecode.py.
//
// A windowed step reads at most W keys wherever the row stands, so everything here follows W and neither the position nor
// the cache length:
//   split     a workgroup is (row, KV HEAD, key range), grid B * Hkv * NS, 256 threads, and serves the G query heads of
//             its K/V head from one read of each K / V row (as decode_gqa.hip).  The NS ranges cut the WINDOW, not the
//             cache: with n = pos - lo + 1 keys, range sp is [lo + sp * ceil(n / NS), ...) -- once the window is full
//             every range has the same ceil(W / NS) keys at every position, the step's time is flat in pos, and the new
//             key's owner is always the last non-empty range.  A key outside [lo, pos] is never read.
//   LDS       [G * hd] rotated queries | [hd] new k | [hd] new v | [64] reductions | max(G * roundup4(chunk) scores,
//             G * groups * hd partial sums), chunk = ceil(min(window, max_len) / NS): a 20000-row cache with a window of
//             64 takes the LDS of a 64-row cache.
//   loads     once the scalar load of the position is back EVERY load is issued, most urgent first -- the new token's G q
//             pair-vectors and its k / v pairs, the cos / sin row, the range's K rows (thread = key; head_dim 48 / 64:
//             the whole row in registers, KPRE), its V rows (thread = (row group, column quad), VPRE) -- none behind a
//             divergent branch, whole-wave skips are uniform; a thread without a key re-reads row t0, inside the window.
//   scores    the G rotated queries sit in LDS (broadcast reads); a thread reads ITS K row once and scores it against all
//             G queries: G accumulators, 4 G FMAs per K float4.  sc[g][key - t0] in LDS.
//   softmax   the G maxima (and later the G sums) are reduced TOGETHER: one pass of wave shuffles over the G-vector, lane 0
//             of each wave leaves G values, one barrier, every thread folds the 4 x G values.
//   P V       a thread reads each of ITS V float4s once and feeds G float4 accumulators.
//   combine   the (row group, g) partial sums go through LDS (the dead score buffer) and are added in a FIXED order -- 8
//             threads per (g, column quad) add every 8th group in place, one thread adds those 8 -- no atomics, no scratch,
//             the same bits on every run.  G records [m, l, -, - | sum exp(s - m) v] leave in the multi-head layout: the
//             consumers (pdn_decode_gemv_f32 act 2, pdn_decode_wide_gemm_f32 mode 3) are unchanged.
// No matrix instruction, for the reason in decode_gqa.hip's header: a workgroup holds at most 8 query rows (here 1 .. 8), an
// MFMA tile would pad them to 16 for nothing, and the work is bandwidth- and latency-bound VALU work (4 G FMAs per 16
// bytes of K against ~11 B/clk per CU).
#include "common.h"
#include "decode_stage.h"

#define BDD_MAX_LDS (60 * 1024)

// floats of LDS in front of the score buffer: [G * hd] rotated queries, [hd] new k, [hd] new v, [64] reductions
static inline __host__ __device__ int bdd_head_floats(int G, int hd) { return G * hd + 2 * hd + 64; }
// the most keys a range ever holds: the window (no longer than the cache) cut into NS
static inline size_t bdd_chunk(int NS, int window, int max_len) {
  const size_t w = (size_t)(window < max_len ? window : max_len);
  return (w + NS - 1) / NS;
}
// the dynamic LDS of a launch: the head, then max(G * chunk scores, G * groups * hd partial sums)
static inline size_t bdd_lds_bytes(int G, int hd, int NS, int window, int max_len) {
  const size_t f4 = hd / 4, groups = 256 / f4, chunk = bdd_chunk(NS, window, max_len);
  const size_t sc = (size_t)G * ((chunk + 3) & ~(size_t)3), comb = (size_t)G * groups * hd;
  return sizeof(float) * ((size_t)bdd_head_floats(G, hd) + (sc > comb ? sc : comb));
}

template <int G, int KPRE, int VPRE>
__global__ __launch_bounds__(256) void bdd_attention_kernel(const int* __restrict__ pos_ptr, int rows, int Hkv, int hd, int NS,
                                                            int window, const float* __restrict__ qkv,
                                                            float* __restrict__ kc, float* __restrict__ vc,
                                                            const float* __restrict__ cs, const float* __restrict__ sn,
                                                            float* __restrict__ part_out, int64_t qkv_rs, int64_t cbs,
                                                            float inv_sqrt) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sp = blockIdx.x % NS, bk = blockIdx.x / NS, b = bk / Hkv, kvh = bk - b * Hkv;
  const int pos_u = rows ? pos_ptr[b] : *pos_ptr;
  const bool keep = pos_u >= 0;                                    // (a stopped row: position 0, no cache byte written)
  const int pos = max(pos_u, 0);
  // the window [lo, pos] (window >= 1, so pos - (window - 1) cannot overflow) and this workgroup's range of it
  const int lo = max(pos - (window - 1), 0), n = pos - lo + 1;
  const int chunk = (n + NS - 1) / NS, t0 = lo + sp * chunk, t1 = min(pos + 1, t0 + chunk);
  const int H = G * Hkv, D = H * hd, KVD = Hkv * hd, f4 = hd / 4, half = hd / 2, rec = 4 + hd;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // the G records of this (row, range, KV head): heads kvh * G .. kvh * G + G - 1 are adjacent
  float* out = part_out + (((int64_t)b * NS + sp) * H + (int64_t)kvh * G) * rec;
  if (t0 >= t1) {                        // no keys in this range (uniform): G x [m = -inf, l = 0, -, - | zeros]
    for (int i = tid; i < G * (rec / 4); i += 256)
      reinterpret_cast<float4*>(out)[i] = (i % (rec / 4)) == 0 ? make_float4(-INFINITY, 0.f, 0.f, 0.f) : z4;
    return;
  }
  float* qs = lds;                       // [G][hd] rotated queries
  float* ks = qs + G * hd;               // [hd] the new key, rotated (the owner's range only)
  float* vs = ks + hd;                   // [hd] the new value
  float* red = vs + hd;                  // [4 waves][G] maxima, then [32 + 4 waves][G] sums
  float* sc = red + 64;                  // [G][cs_] scores, then the partial sums of the combine
  const int cs_ = (chunk + 3) & ~3;      // (chunk <= ceil(min(window, max_len) / NS): the launch's LDS holds it)
  float* kb = kc + (int64_t)b * cbs + (int64_t)kvh * hd;
  float* vb = vc + (int64_t)b * cbs + (int64_t)kvh * hd;
  const bool owner = pos < t1;           // (pos >= t0 here: the last non-empty range)

  // ---- every load of the kernel, most urgent first (threads without a pair / a row re-read a valid one) ----
  const float* row = qkv + (int64_t)b * qkv_rs;
  const int nqp = G * half;                                        // q pairs of the group: <= 512, two per thread
  const int qi0 = min(tid, nqp - 1), qi1 = min(tid + 256, nqp - 1);
  const float2 nq0 = *reinterpret_cast<const float2*>(row + (unsigned)(kvh * G * hd + 2 * qi0));
  float2 nq1 = make_float2(0.f, 0.f);
  if (nqp > 256) nq1 = *reinterpret_cast<const float2*>(row + (unsigned)(kvh * G * hd + 2 * qi1));
  const int hq = min(tid, half - 1);                               // the k / v pair of thread tid < hd / 2
  const float2 nk = *reinterpret_cast<const float2*>(row + (unsigned)(D + kvh * hd + 2 * hq));
  const float2 nv = *reinterpret_cast<const float2*>(row + (unsigned)(D + KVD + kvh * hd + 2 * hq));
  const int j0 = qi0 % half, j1 = qi1 % half;
  const float c0 = cs[(unsigned)(pos * half + j0)], s0 = sn[(unsigned)(pos * half + j0)];
  float c1 = 0.f, s1 = 0.f;
  if (nqp > 256) { c1 = cs[(unsigned)(pos * half + j1)]; s1 = sn[(unsigned)(pos * half + j1)]; }
  const float ck = cs[(unsigned)(pos * half + hq)], sk = sn[(unsigned)(pos * half + hq)];
  float4 kreg[KPRE > 0 ? KPRE : 1];
  const int kt = t0 + tid;                                         // the key this thread scores first
  if (KPRE > 0 && t0 + (tid & ~63) < t1) {                         // (uniform per wave: this wave has a key)
    // (a thread without a key, or with the new one, reads row t0: t0 is in [lo, pos], never a row outside the window)
    const float* kp = kb + (unsigned)(((kt < t1 && kt != pos) ? kt : t0) * KVD);
#pragma unroll
    for (int c = 0; c < KPRE; ++c) kreg[c] = *reinterpret_cast<const float4*>(kp + 4 * c);
  }
  const int groups = dec_div(256, f4), tg = dec_div(tid, f4), vc4 = tid - tg * f4;
  float4 vreg[VPRE > 0 ? VPRE : 1];
  if (VPRE > 0) {
    const int nv_rows = __builtin_amdgcn_readfirstlane((t1 - t0 + groups - 1) / groups);     // row steps with any key
#pragma unroll
    for (int i = 0; i < VPRE; ++i) {
      const int t = t0 + tg + i * groups;
      if (i < nv_rows)
        vreg[i] = *reinterpret_cast<const float4*>(vb + (unsigned)(((t < t1 && t != pos) ? t : t0) * KVD + 4 * vc4));
    }
  }

  // ---- RoPE (interleaved pairs) of the G queries -> LDS; the owner rotates k and appends k / v to cache row pos ----
  if (tid < nqp) *reinterpret_cast<float2*>(qs + 2 * tid) = make_float2(nq0.x * c0 - nq0.y * s0, nq0.x * s0 + nq0.y * c0);
  if (tid + 256 < nqp)
    *reinterpret_cast<float2*>(qs + 2 * (tid + 256)) = make_float2(nq1.x * c1 - nq1.y * s1, nq1.x * s1 + nq1.y * c1);
  if (owner && tid < half) {
    const float2 kr = make_float2(nk.x * ck - nk.y * sk, nk.x * sk + nk.y * ck);
    *reinterpret_cast<float2*>(ks + 2 * tid) = kr;
    *reinterpret_cast<float2*>(vs + 2 * tid) = nv;
    if (keep) {
      *reinterpret_cast<float2*>(kb + (int64_t)pos * KVD + 2 * tid) = kr;
      *reinterpret_cast<float2*>(vb + (int64_t)pos * KVD + 2 * tid) = nv;
    }
  }
  lds_barrier();

  // ---- scores: each K row read once, scored against the G queries ----
  const float4* q4 = reinterpret_cast<const float4*>(qs);
  float m[G];
#pragma unroll
  for (int g = 0; g < G; ++g) m[g] = -INFINITY;
  for (int t = kt; t < t1; t += 256) {
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = 0.f;
    if (KPRE > 0 && t == kt && t != pos) {
#pragma unroll
      for (int c = 0; c < KPRE; ++c) {
        const float4 k = kreg[c];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float4 a = q4[g * KPRE + c];
          s[g] += (a.x * k.x + a.y * k.y) + (a.z * k.z + a.w * k.w);
        }
      }
    } else {
      const float4* k4 = t == pos ? reinterpret_cast<const float4*>(ks)
                                  : reinterpret_cast<const float4*>(kb + (unsigned)(t * KVD));
      for (int c = 0; c < f4; ++c) {
        const float4 k = k4[c];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float4 a = q4[g * f4 + c];
          s[g] += (a.x * k.x + a.y * k.y) + (a.z * k.z + a.w * k.w);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      s[g] *= inv_sqrt;
      sc[g * cs_ + (t - t0)] = s[g];
      m[g] = fmaxf(m[g], s[g]);
    }
  }
  // the G maxima together: shuffles over the G-vector, then the four waves through LDS
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) m[g] = fmaxf(m[g], __shfl_xor(m[g], o, 64));
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) red[wave * G + g] = m[g];
  }
  lds_barrier();
#pragma unroll
  for (int g = 0; g < G; ++g) m[g] = fmaxf(fmaxf(red[g], red[G + g]), fmaxf(red[2 * G + g], red[3 * G + g]));

  // ---- probabilities (each thread rewrites the scores it wrote) and the G sums ----
  float l[G];
#pragma unroll
  for (int g = 0; g < G; ++g) l[g] = 0.f;
  for (int t = kt; t < t1; t += 256) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float pr = expf(sc[g * cs_ + (t - t0)] - m[g]);
      sc[g * cs_ + (t - t0)] = pr;
      l[g] += pr;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) l[g] += __shfl_xor(l[g], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) red[32 + wave * G + g] = l[g];      // (behind the maxima: 4 * G <= 32)
  }
  lds_barrier();                         // (publishes the probabilities too)
#pragma unroll
  for (int g = 0; g < G; ++g) l[g] = (red[32 + g] + red[32 + G + g]) + (red[32 + 2 * G + g] + red[32 + 3 * G + g]);

  // ---- P V: each V float4 read once, G accumulators ----
  float4 acc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) acc[g] = z4;
  if (tg < groups) {
    if (VPRE > 0) {
#pragma unroll
      for (int i = 0; i < VPRE; ++i) {
        const int t = t0 + tg + i * groups;
        if (t < t1) {
          const float4 v = t == pos ? reinterpret_cast<const float4*>(vs)[vc4] : vreg[i];
#pragma unroll
          for (int g = 0; g < G; ++g) {
            const float pr = sc[g * cs_ + (t - t0)];
            acc[g].x += pr * v.x; acc[g].y += pr * v.y; acc[g].z += pr * v.z; acc[g].w += pr * v.w;
          }
        }
      }
    }
    for (int t = t0 + tg + VPRE * groups; t < t1; t += groups) {
      const float4 v = t == pos ? reinterpret_cast<const float4*>(vs)[vc4]
                                : *reinterpret_cast<const float4*>(vb + (unsigned)(t * KVD + 4 * vc4));
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float pr = sc[g * cs_ + (t - t0)];
        acc[g].x += pr * v.x; acc[g].y += pr * v.y; acc[g].z += pr * v.z; acc[g].w += pr * v.w;
      }
    }
  }
  lds_barrier();                         // the probabilities are dead: the buffer takes the partial sums
  float4* part = reinterpret_cast<float4*>(sc);                    // [G][groups][f4]
  if (tg < groups) {
#pragma unroll
    for (int g = 0; g < G; ++g) part[(g * groups + tg) * f4 + vc4] = acc[g];
  }
  lds_barrier();
  // combine in a fixed order: 8 threads per (g, column quad) add every 8th group into the first (only they read it),
  // then one thread adds those 8 (groups = 256 / f4 >= 8 up to head_dim 128)
  for (int s = tid; s < G * 8 * f4; s += 256) {
    const int g = s / (8 * f4), r8 = s - g * 8 * f4, g0 = r8 / f4, c4 = r8 - g0 * f4;
    float4 r = part[(g * groups + g0) * f4 + c4];
    for (int gg = g0 + 8; gg < groups; gg += 8) {
      const float4 t = part[(g * groups + gg) * f4 + c4];
      r.x += t.x; r.y += t.y; r.z += t.z; r.w += t.w;
    }
    part[(g * groups + g0) * f4 + c4] = r;
  }
  lds_barrier();
  if (tid < G * f4) {
    const int g = tid / f4, c4 = tid - g * f4;
    float4 r = part[(g * groups) * f4 + c4];
    for (int g0 = 1; g0 < 8; ++g0) {
      const float4 t = part[(g * groups + g0) * f4 + c4];
      r.x += t.x; r.y += t.y; r.z += t.z; r.w += t.w;
    }
    reinterpret_cast<float4*>(out + (unsigned)(g * rec) + 4)[c4] = r;
  }
  if (tid == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) { out[g * rec] = m[g]; out[g * rec + 1] = l[g]; }
  }
}

namespace {
bool bdd_shape_ok(int H, int Hkv, int head_dim, int n_splits, int window, int max_len) {
  if (H <= 0 || Hkv <= 0 || H % Hkv || H / Hkv > 8) return false;
  if (head_dim <= 0 || head_dim % 4 || head_dim > 128 || n_splits < 1 || n_splits > 64) return false;
  if (window < 1 || max_len <= 0) return false;
  return bdd_lds_bytes(H / Hkv, head_dim, n_splits, window, max_len) <= BDD_MAX_LDS;
}

template <int G>
void bdd_launch(dim3 grid, size_t shm, hipStream_t st, const int* pos, int rows, int Hkv, int hd, int NS, int window,
                const float* qkv, float* kc, float* vc, const float* cs, const float* sn, float* parts, int64_t qkv_rs,
                int64_t cbs, float inv_sqrt) {
#define BDD_GO(KP, VP)                                                                                                  \
  hipLaunchKernelGGL((bdd_attention_kernel<G, KP, VP>), grid, dim3(256), shm, st, pos, rows, Hkv, hd, NS, window, qkv, kc, \
                     vc, cs, sn, parts, qkv_rs, cbs, inv_sqrt)
  if (hd == 48) BDD_GO(12, 13);
  else if (hd == 64) BDD_GO(16, 16);
  else BDD_GO(0, 0);
#undef BDD_GO
}
}  // namespace

extern "C" {

int pdnv_decode_attention_supported(int H, int Hkv, int head_dim, int n_splits, int window, int max_len) {
  return bdd_shape_ok(H, Hkv, head_dim, n_splits, window, max_len) ? 1 : 0;
}

int pdnv_decode_attention_f32(const float* qkv, int64_t qkv_row_stride, const float* cos_table, const float* sin_table,
                              float* k_cache, float* v_cache, float* partials, int B, int H, int Hkv, int head_dim,
                              int n_splits, int64_t cache_batch_stride, const int* pos, int max_len, int window, int rows,
                              void* stream) {
  if (B == 0 || H == 0) return PDN_OK;
  PDN_CHECK_ARG(qkv && cos_table && sin_table && k_cache && v_cache && partials && pos && max_len > 0 && B > 0,
                "pdnv_decode_attention_f32: bad arguments");
  if (!bdd_shape_ok(H, Hkv, head_dim, n_splits, window, max_len)) {
    pdn_set_error("pdnv_decode_attention_f32: %d heads over %d key/value heads (group 1 .. 8), head_dim %d (%% 4, <= 128), "
                  "%d ranges of a window of %d keys (>= 1) in max_len %d: outside pdnv_decode_attention_supported", H, Hkv,
                  head_dim, n_splits, window, max_len);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG((cache_batch_stride % 4) == 0 && qkv_row_stride % 4 == 0 &&
                    ((((uintptr_t)qkv | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)partials) & 15) == 0),
                "pdnv_decode_attention_f32: 16-byte alignment required");
  const int G = H / Hkv, KVD = Hkv * head_dim;
  const int64_t lim = (int64_t)1 << 31;
  PDN_CHECK_ARG((int64_t)max_len * KVD < lim && (int64_t)H * head_dim + 2 * (int64_t)KVD < lim &&
                    (int64_t)max_len * (head_dim / 2) < lim && (int64_t)B * Hkv * n_splits < lim &&
                    qkv_row_stride >= (int64_t)H * head_dim + 2 * (int64_t)KVD && cache_batch_stride >= (int64_t)max_len * KVD,
                "pdnv_decode_attention_f32: rows out of the 32-bit range of the kernel, or strides shorter than a row");
  // (a window past the cache is the whole cache: plain causal decode attention; the kernel's lo clamps at 0 either way)
  const int W = window < max_len ? window : max_len;
  const size_t shm = bdd_lds_bytes(G, head_dim, n_splits, W, max_len);
  const dim3 grid((unsigned)(B * Hkv * n_splits));
  const float inv_sqrt = 1.f / sqrtf((float)head_dim);
  hipStream_t st = (hipStream_t)stream;
#define BDD_G(N)                                                                                                        \
  case N:                                                                                                               \
    bdd_launch<N>(grid, shm, st, pos, rows ? 1 : 0, Hkv, head_dim, n_splits, W, qkv, k_cache, v_cache, cos_table,         \
                  sin_table, partials, qkv_row_stride, cache_batch_stride, inv_sqrt);                                   \
    break
  switch (G) {
    BDD_G(1); BDD_G(2); BDD_G(3); BDD_G(4); BDD_G(5); BDD_G(6); BDD_G(7); BDD_G(8);
  }
#undef BDD_G
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_BAND);
  return PDN_OK;
}

}  // extern "C"
