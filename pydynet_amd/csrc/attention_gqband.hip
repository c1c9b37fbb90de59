// Sliding-window attention over grouped heads (forward + backward) for gfx950, fp32 MFMA -- the Mistral layer: H query heads
// share Hkv < H key/value heads (query head h reads key/value head h / G, G = H / Hkv in 2 .. 8), and query i, at absolute
// position i + start_pos, sees the keys max(0, i + start_pos - W + 1) .. i + start_pos of that head.  Operands as in
// attention_band.hip and attention_gqa.hip -- any Lq, Lk >= start_pos + Lq, separate q and k/v strides, head dims 16 .. 128
// -- and the same transposed-score scheme (attention_tile.h): a lane owns a query, the softmax is in-lane, P^T feeds the next
// MFMA from registers, 32-row tiles arrive through a double-buffered LDS ring.  Statements: core/fused/band.py over
// core/fused/gqa.py.  No mask operand, no bounds buffer; K and V are never expanded, neither in HBM nor in LDS.
//
// The work split is the grouped kernels' unit numbering laid over the band kernels' key ranges:
//   forward, dQ   the unit is one (head of the group, 32-query tile) pair, heads fastest: u = tile * G + g.  A workgroup of
//                 four wave64 takes four consecutive units of ONE (batch, KV head).  Each wave derives the key tiles
//                 [my_lo, my_hi] of its own query tile -- from the tile of its first query's lowest visible key to the tile
//                 of its last query's own key -- and the workgroup stages the union, from my_lo of wave 0 to my_hi of the
//                 last live wave (both ascend with the unit), ONCE through the ring.  A wave skips the products of a staged
//                 tile outside its range and still loads its share of every tile and takes every barrier.  With G >= 4 the
//                 four waves sit at one or two adjacent query tiles: the union is ceil(W / 32) + 1 .. 3 tiles where the
//                 plain band kernels stage + 4 .. 5 for their four consecutive tiles, no wave idles through more than one
//                 staged tile, and every staged tile feeds up to four heads.  With G = 2: two tiles x two heads.
//                 Grid (ceil(G * ceil(Lq / 32) / 4), B * Hkv).
//   dK/dV         a workgroup owns 4 x 32 key rows of one (batch, KV head) and keeps dK^T, dV^T in accumulators while the
//                 Q / dO tiles that can see those keys -- queries k_first - start_pos .. k_last + W - 1 - start_pos, for every
//                 head of the group, head-major -- stream through the ring with their lse and delta; each wave skips the
//                 query tiles outside its own 32 keys' range.  The sum over the group is the accumulator itself: one store at
//                 the end in a fixed order, no atomics, no expanded gradients, the same bits on every run, and zeros for
//                 keys no query sees.  Grid (ceil(Lk / 128), B * Hkv).
// The elementwise test (key below the lower edge, key above the query) runs on a wave's EDGE tiles only, on wave-uniform
// values, as in attention_band.hip; for W < 32 or start_pos % 32 != 0 both edges can fall into one tile, which takes both.
#include "attention_tile.h"

struct GqBandArgs {
  AttnArgs a;       // H = query heads, causal = 1; mask / rc / rs unused
  int W;            // the window, clipped by the host to start_pos + Lq (a wider one is plain causal attention)
  int Hkv, G;
};

// the unit of wave `wave` of workgroup blockIdx.x -- query tile and head of the group -- and the key tiles it needs
struct GqBandSpan {
  int qt0, g;
  bool live;
  int q_lo, q_hi;        // absolute positions of the unit's first and last (existing) query
  int my_lo, my_hi;      // key tiles this wave consumes (my_hi = -1: none)
  int kt_lo, kt_hi;      // key tiles the workgroup stages
};

__device__ __forceinline__ GqBandSpan gqband_span(const GqBandArgs& ga, int wave) {
  const AttnArgs& a = ga.a;
  const int units = ga.G * ((a.Lq + 31) / 32), u0 = blockIdx.x * 4, u = u0 + wave;
  GqBandSpan s;
  s.live = u < units;                                      // wave-uniform
  const int uc = min(u, units - 1), qt = uc / ga.G;        // (a wave past the last unit sits at the last one and stores nothing)
  s.g = uc - qt * ga.G;
  s.qt0 = qt * 32;                                         // < Lq
  s.q_lo = s.qt0 + a.start_pos;
  s.q_hi = min(s.qt0 + 31, a.Lq - 1) + a.start_pos;
  s.my_lo = max(0, s.q_lo - ga.W + 1) / 32;
  s.my_hi = s.live ? s.q_hi / 32 : -1;
  // both ends ascend with the unit: the union is [lowest tile of wave 0, diagonal tile of the last live wave]
  const int qt_first = u0 / ga.G, qt_last = min(u0 + 3, units - 1) / ga.G;
  s.kt_lo = max(0, qt_first * 32 + a.start_pos - ga.W + 1) / 32;
  s.kt_hi = (min(qt_last * 32 + 31, a.Lq - 1) + a.start_pos) / 32;      // < ceil(Lk / 32): Lk >= start_pos + Lq
  return s;
}

// whether key tile kt holds a key that some query of the unit does not see
__device__ __forceinline__ bool gqband_edge(const GqBandSpan& s, int W, int kt) {
  return kt * 32 < s.q_hi - W + 1 || kt * 32 + 31 > s.q_lo;
}

// ---- forward ------------------------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void gqband_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                         const float* __restrict__ V, float* __restrict__ O,
                                                         float* __restrict__ LSE, GqBandArgs ga) {
  constexpr int LD = AS_LD(HD), NT8 = HD / 8, F4 = HD / 4, DT = (HD + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  auto Kbuf = [&](int i) { return lds + (i & 1) * (2 * 32 * LD); };
  auto Vbuf = [&](int i) { return lds + (i & 1) * (2 * 32 * LD) + 32 * LD; };
  const AttnArgs& a = ga.a;
  const int bj = blockIdx.y, b = bj / ga.Hkv, j = bj - b * ga.Hkv;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const GqBandSpan w = gqband_span(ga, wave);
  const int h = j * ga.G + w.g, bh = b * a.H + h, qt0 = w.qt0;
  const float* Qb = Q + (int64_t)b * a.q_bs + (int64_t)h * HD;
  const float* Kg = K + (int64_t)b * a.kv_bs + (int64_t)j * HD;
  const float* Vg = V + (int64_t)b * a.kv_bs + (int64_t)j * HD;
  float* Ob = O + (int64_t)b * a.q_bs + (int64_t)h * HD;
  // a lane past Lq computes the last query over again and stores nothing: no row is ever fully masked
  const int qpos = qt0 + li, qc = min(qpos, a.Lq - 1), qabs = qc + a.start_pos, qlow = qabs - ga.W + 1;

  TileLoader<HD> ld;
  ld.issue(Kg, Vg, a.kv_rs, w.kt_lo * 32, a.Lk, nullptr, nullptr, false);
  ld.commit(Kbuf(0), Vbuf(0));
  // Q fragments: lane (li, lh) holds Q[q][8t + 4lh .. +3]
  float4 qf[NT8];
  {
    const float* qrow = Qb + (int64_t)qc * a.q_rs + 4 * lh;
#pragma unroll
    for (int t = 0; t < NT8; ++t) qf[t] = *reinterpret_cast<const float4*>(qrow + 8 * t);
  }
  f32x16 o[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  __syncthreads();
  for (int kt = w.kt_lo; kt <= w.kt_hi; ++kt) {
    const int it = kt - w.kt_lo;
    if (kt < w.kt_hi) ld.issue(Kg, Vg, a.kv_rs, (kt + 1) * 32, a.Lk, nullptr, nullptr, false);
    if (kt >= w.my_lo && kt <= w.my_hi) {
      const float* Ks = Kbuf(it);
      const float* Vs = Vbuf(it);
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      const float* krow = Ks + li * LD + 4 * lh;
#pragma unroll
      for (int t = 0; t < NT8; ++t) {
        const float4 kf = *reinterpret_cast<const float4*>(krow + 8 * t);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[t].x, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[t].y, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[t].z, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[t].w, s, 0, 0, 0);
      }
      const bool edge = gqband_edge(w, ga.W, kt);                // wave-uniform: interior tiles run unmasked
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = s[r] * a.inv_sqrt;
        if (edge) {
          const int key = kt * 32 + as_krow(r, lh);             // (key > qabs covers the keys past Lk: qabs < Lk)
          if (key < qlow || key > qabs) v = -INFINITY;
        }
        s[r] = v;
        tm = fmaxf(tm, v);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      const float mn = fmaxf(m, tm);
      // rows that have seen only -inf so far keep p = 0 and an unscaled (zero) accumulator
      const float alpha = mn == -INFINITY ? 1.f : __expf(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = mn == -INFINITY ? 0.f : __expf(s[r] - mn);
        s[r] = p;
        ps += p;
      }
      l = l * alpha + ps;
      m = mn;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vrow = Vs + as_krow(r, lh) * LD + li;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const float av = (d * 32 + 32 <= HD || d * 32 + li < HD) ? vrow[d * 32] : 0.f;
          o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, s[r], o[d], 0, 0, 0);
        }
      }
    }
    if (kt < w.kt_hi) ld.commit(Kbuf(it + 1), Vbuf(it + 1));
    __syncthreads();
  }
  // ---- normalise, stage [q][d] through this wave's quarter of the ring, store rows coalesced -------
  l += __shfl_xor(l, 32, 64);
  const float inv_l = 1.f / l;
  float* Ow = lds + wave * 32 * LD;
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dd = d * 32 + as_krow(r, lh);
      if (dd < HD) Ow[li * LD + dd] = o[d][r] * inv_l;
    }
  const int n_rows = w.live ? a.Lq : 0;             // a wave past the last unit stores nothing
  if (lh == 0 && qpos < n_rows) LSE[(int64_t)bh * a.Lq + qpos] = m + logf(l);
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  for (int u = lane; u < 32 * F4; u += 64) {
    const int row = u / F4, c4 = u - row * F4;
    if (qt0 + row < n_rows)
      *reinterpret_cast<float4*>(Ob + (int64_t)(qt0 + row) * a.q_rs + 4 * c4) =
          *reinterpret_cast<const float4*>(Ow + row * LD + 4 * c4);
  }
}

// ---- backward: dQ (and delta) ---------------------------------------------------------------------
template <int HD>
__global__ __launch_bounds__(256) void gqband_bwd_dq_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ O, const float* __restrict__ dO, const float* __restrict__ LSE,
    float* __restrict__ dQ, float* __restrict__ Delta, GqBandArgs ga) {
  constexpr int LD = AS_LD(HD), NT8 = HD / 8, DT = (HD + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  auto Kbuf = [&](int i) { return lds + (i & 1) * (2 * 32 * LD); };
  auto Vbuf = [&](int i) { return lds + (i & 1) * (2 * 32 * LD) + 32 * LD; };
  const AttnArgs& a = ga.a;
  const int bj = blockIdx.y, b = bj / ga.Hkv, j = bj - b * ga.Hkv;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const GqBandSpan w = gqband_span(ga, wave);
  const int h = j * ga.G + w.g, bh = b * a.H + h, qt0 = w.qt0;
  const int64_t qbase = (int64_t)b * a.q_bs + (int64_t)h * HD;
  const float* Kg = K + (int64_t)b * a.kv_bs + (int64_t)j * HD;
  const float* Vg = V + (int64_t)b * a.kv_bs + (int64_t)j * HD;
  const int qpos = qt0 + li, qc = min(qpos, a.Lq - 1), qabs = qc + a.start_pos, qlow = qabs - ga.W + 1;
  TileLoader<HD> ld;
  ld.issue(Kg, Vg, a.kv_rs, w.kt_lo * 32, a.Lk, nullptr, nullptr, false);
  ld.commit(Kbuf(0), Vbuf(0));
  // delta = dO . o from the SAME contraction as dP = dO . v below (the diagonal of O dO^T), as in attention_stream.hip:
  // where a row sees one key (W = 1: o = v) dP - delta cancels to an exact zero
  float4 qf[NT8], gf[NT8];
  f32x16 dd;
#pragma unroll
  for (int r = 0; r < 16; ++r) dd[r] = 0.f;
  {
    const float* qrow = Q + qbase + (int64_t)qc * a.q_rs + 4 * lh;
    const float* grow = dO + qbase + (int64_t)qc * a.q_rs + 4 * lh;
    const float* orow = O + qbase + (int64_t)qc * a.q_rs + 4 * lh;
#pragma unroll
    for (int t = 0; t < NT8; ++t) {
      qf[t] = *reinterpret_cast<const float4*>(qrow + 8 * t);
      gf[t] = *reinterpret_cast<const float4*>(grow + 8 * t);
      const float4 ov = *reinterpret_cast<const float4*>(orow + 8 * t);
      dd = __builtin_amdgcn_mfma_f32_32x32x2f32(ov.x, gf[t].x, dd, 0, 0, 0);
      dd = __builtin_amdgcn_mfma_f32_32x32x2f32(ov.y, gf[t].y, dd, 0, 0, 0);
      dd = __builtin_amdgcn_mfma_f32_32x32x2f32(ov.z, gf[t].z, dd, 0, 0, 0);
      dd = __builtin_amdgcn_mfma_f32_32x32x2f32(ov.w, gf[t].w, dd, 0, 0, 0);
    }
  }
  // dd[r] of lane (li, lh) is o[as_krow(r, lh)] . dO[li]: the diagonal sits in the half-wave with lh = bit 2 of li
  float dpart = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (r == (li & 3) + 4 * (li >> 3)) dpart = dd[r];
  const float dother = __shfl_xor(dpart, 32, 64);
  const float delta_q = lh == ((li >> 2) & 1) ? dpart : dother;
  const float lse_q = LSE[(int64_t)bh * a.Lq + qc];
  const int n_rows = w.live ? a.Lq : 0;             // a wave past the last unit stores nothing
  if (lh == 0 && qpos < n_rows) Delta[(int64_t)bh * a.Lq + qpos] = delta_q;
  f32x16 dq[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[d][r] = 0.f;
  __syncthreads();
  for (int kt = w.kt_lo; kt <= w.kt_hi; ++kt) {
    const int it = kt - w.kt_lo;
    if (kt < w.kt_hi) ld.issue(Kg, Vg, a.kv_rs, (kt + 1) * 32, a.Lk, nullptr, nullptr, false);
    if (kt >= w.my_lo && kt <= w.my_hi) {
      const float* Ks = Kbuf(it);
      const float* Vs = Vbuf(it);
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
      const float* krow = Ks + li * LD + 4 * lh;
      const float* vrow = Vs + li * LD + 4 * lh;
#pragma unroll
      for (int t = 0; t < NT8; ++t) {
        const float4 kf = *reinterpret_cast<const float4*>(krow + 8 * t);
        const float4 vf = *reinterpret_cast<const float4*>(vrow + 8 * t);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[t].x, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.x, gf[t].x, dp, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[t].y, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.y, gf[t].y, dp, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[t].z, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.z, gf[t].z, dp, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[t].w, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.w, gf[t].w, dp, 0, 0, 0);
      }
      // dS^T[key][q] = P^T o (dP^T - delta_q) / sqrt(hd)   (lane = q)
      const bool edge = gqband_edge(w, ga.W, kt);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + as_krow(r, lh);
        const bool out = edge && (key < qlow || key > qabs);
        const float p = out ? 0.f : __expf(s[r] * a.inv_sqrt - lse_q);
        s[r] = p * (dp[r] - delta_q) * a.inv_sqrt;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* kr = Ks + as_krow(r, lh) * LD + li;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const float av = (d * 32 + 32 <= HD || d * 32 + li < HD) ? kr[d * 32] : 0.f;
          dq[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, s[r], dq[d], 0, 0, 0);
        }
      }
    }
    if (kt < w.kt_hi) ld.commit(Kbuf(it + 1), Vbuf(it + 1));
    __syncthreads();
  }
  as_store_T<HD, DT>(lds + wave * 32 * LD, dq, dQ + qbase, a.q_rs, qt0, n_rows, li, lh, lane, nullptr, nullptr, 0);
}

// ---- backward: dK, dV ------------------------------------------------------------------------------
// K, V fragments of 4 x 32 key rows in registers; the (head of the group, query tile) pairs that can see them stream
// through the ring head-major.  S[q][key] = Q K^T: lane = key, registers = queries.
template <int HD>
__global__ __launch_bounds__(256) void gqband_bwd_dkv_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ dO, const float* __restrict__ LSE, const float* __restrict__ Delta,
    float* __restrict__ dK, float* __restrict__ dV, GqBandArgs ga) {
  constexpr int LD = AS_LD(HD), NT8 = HD / 8, DT = (HD + 31) / 32;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  auto Qbuf = [&](int i) { return lds + (i & 1) * (2 * 32 * LD); };
  auto Gbuf = [&](int i) { return lds + (i & 1) * (2 * 32 * LD) + 32 * LD; };
  float* stat = lds + 4 * 32 * LD;                  // [2 buffers][lse 32 | delta 32]
  const AttnArgs& a = ga.a;
  const int bj = blockIdx.y, b = bj / ga.Hkv, j = bj - b * ga.Hkv, h0 = j * ga.G;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
  const int k0 = blockIdx.x * 128, kt0 = k0 + wave * 32;
  const int64_t kbase = (int64_t)b * a.kv_bs + (int64_t)j * HD;
  const float* Qg = Q + (int64_t)b * a.q_bs + (int64_t)h0 * HD;        // head g of the group: + g * HD
  const float* Gg = dO + (int64_t)b * a.q_bs + (int64_t)h0 * HD;
  const int64_t sbase = ((int64_t)b * a.H + h0) * a.Lq;                // lse / delta row of head g: + g * Lq
  const int kpos = kt0 + li, kc = min(kpos, a.Lk - 1);
  // query tiles that see the keys [kf, kl]: kf - start_pos <= q <= kl + W - 1 - start_pos, clipped to [0, Lq); last < first: none
  auto tiles = [&](int kf, int kl, int& first, int& last) {
    const int64_t ql = min((int64_t)a.Lq - 1, (int64_t)kl + ga.W - 1 - a.start_pos);
    const int64_t qf = max((int64_t)0, (int64_t)kf - a.start_pos);
    first = ql < qf ? 0 : (int)(qf / 32);
    last = ql < qf ? -1 : (int)(ql / 32);
  };
  int qt_first, qt_last, my_first, my_last;         // the workgroup's stream per head, this wave's part of it (wave-uniform)
  tiles(k0, min(k0 + 127, a.Lk - 1), qt_first, qt_last);
  tiles(kt0, min(kt0 + 31, a.Lk - 1), my_first, my_last);
  if (kt0 >= a.Lk) my_last = -1;
  const int total = ga.G * (qt_last - qt_first + 1);                   // (head, tile) pairs to stream; 0: none
  TileLoader<HD> ld;
  auto load_stats = [&](int g, int qt, int buf) {
    if (threadIdx.x < 64) {
      const int q = qt * 32 + (threadIdx.x & 31);
      const float* src = threadIdx.x < 32 ? LSE : Delta;
      stat[buf * 64 + threadIdx.x] = q < a.Lq ? src[sbase + (int64_t)g * a.Lq + q] : 0.f;
    }
  };
  if (total > 0) {
    ld.issue(Qg, Gg, a.q_rs, qt_first * 32, a.Lq, nullptr, nullptr, false);
    ld.commit(Qbuf(0), Gbuf(0));
    load_stats(0, qt_first, 0);
  }
  float4 kf[NT8], vf[NT8];
  {
    const float* krow = K + kbase + (int64_t)kc * a.kv_rs + 4 * lh;
    const float* vrow = V + kbase + (int64_t)kc * a.kv_rs + 4 * lh;
#pragma unroll
    for (int t = 0; t < NT8; ++t) {
      kf[t] = *reinterpret_cast<const float4*>(krow + 8 * t);
      vf[t] = *reinterpret_cast<const float4*>(vrow + 8 * t);
    }
  }
  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[d][r] = 0.f; dv[d][r] = 0.f; }
  __syncthreads();
  for (int it = 0, g = 0, qt = qt_first; it < total; ++it) {
    int gn = g, qn = qt + 1;                        // the pair after this one: next tile, or the next head's first
    if (qn > qt_last) { qn = qt_first; gn = g + 1; }
    if (it + 1 < total) ld.issue(Qg + gn * HD, Gg + gn * HD, a.q_rs, qn * 32, a.Lq, nullptr, nullptr, false);
    if (qt >= my_first && qt <= my_last) {
      const float* Qs = Qbuf(it);
      const float* Gs = Gbuf(it);
      const float* st = stat + (it & 1) * 64;
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
      const float* qrow = Qs + li * LD + 4 * lh;
      const float* grow = Gs + li * LD + 4 * lh;
#pragma unroll
      for (int t = 0; t < NT8; ++t) {
        const float4 q4 = *reinterpret_cast<const float4*>(qrow + 8 * t);
        const float4 g4 = *reinterpret_cast<const float4*>(grow + 8 * t);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.x, kf[t].x, s, 0, 0, 0);      // S[q][key]
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(g4.x, vf[t].x, dp, 0, 0, 0);    // dP[q][key]
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.y, kf[t].y, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(g4.y, vf[t].y, dp, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.z, kf[t].z, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(g4.z, vf[t].z, dp, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(q4.w, kf[t].w, s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(g4.w, vf[t].w, dp, 0, 0, 0);
      }
      // lane = key, registers = queries.  Edge tiles: a key above the tile's first query or below the lower edge of its last
      // one, a query past Lq or a key past Lk
      const int qa0 = qt * 32 + a.start_pos;
      const bool edge = kt0 + 31 > qa0 || kt0 < qa0 + 31 - ga.W + 1 || qt * 32 + 31 >= a.Lq || kt0 + 31 >= a.Lk;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qr = as_krow(r, lh), qabs = qa0 + qr;
        const bool out = edge && (qt * 32 + qr >= a.Lq || kpos >= a.Lk || kpos > qabs || kpos < qabs - ga.W + 1);
        const float p = out ? 0.f : __expf(s[r] * a.inv_sqrt - st[qr]);
        s[r] = p;                                               // P[q][key]
        dp[r] = p * (dp[r] - st[32 + qr]) * a.inv_sqrt;         // dS[q][key]
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qr = as_krow(r, lh);
        const float* gr = Gs + qr * LD + li;
        const float* qq = Qs + qr * LD + li;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const bool ok = d * 32 + 32 <= HD || d * 32 + li < HD;
          const float g0 = ok ? gr[d * 32] : 0.f, q0v = ok ? qq[d * 32] : 0.f;
          dv[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(g0, s[r], dv[d], 0, 0, 0);      // dV^T += dO^T P
          dk[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(q0v, dp[r], dk[d], 0, 0, 0);    // dK^T += Q^T dS
        }
      }
    }
    if (it + 1 < total) {
      ld.commit(Qbuf(it + 1), Gbuf(it + 1));
      load_stats(gn, qn, (it + 1) & 1);
    }
    __syncthreads();
    g = gn;
    qt = qn;
  }
  // (a wave whose keys no query sees stores the zeros it started from)
  float* slot = lds + wave * 32 * LD;
  as_store_T<HD, DT>(slot, dk, dK + kbase, a.kv_rs, kt0, a.Lk, li, lh, lane, nullptr, nullptr, 0);
  as_store_T<HD, DT>(slot, dv, dV + kbase, a.kv_rs, kt0, a.Lk, li, lh, lane, nullptr, nullptr, 0);
}

// ---- host ---------------------------------------------------------------------------------------------
namespace {
int64_t gqband_lds(int hd) { return 4ll * (4 * 32 * AS_LD(hd) + 128); }

// every head dim and group size of the grouped kernels: the register budget is theirs (no operand is added)
bool gqband_hd_ok(int hd) { return hd == 16 || hd == 24 || hd == 32 || hd == 48 || hd == 64 || hd == 96 || hd == 128; }

bool gqband_group_ok(int H, int Hkv) { return Hkv > 0 && H > 0 && H % Hkv == 0 && H / Hkv >= 2 && H / Hkv <= 8; }

#define GQBAND_DISPATCH(HDV, BODY)                   \
  switch (HDV) {                                     \
    case 16: { constexpr int HD = 16; BODY; } break; \
    case 24: { constexpr int HD = 24; BODY; } break; \
    case 32: { constexpr int HD = 32; BODY; } break; \
    case 48: { constexpr int HD = 48; BODY; } break; \
    case 64: { constexpr int HD = 64; BODY; } break; \
    case 96: { constexpr int HD = 96; BODY; } break; \
    default: { constexpr int HD = 128; BODY; } break; \
  }

// B * Hkv is the grid's y extent, held to the 65535 of the streaming entries
constexpr int64_t kGqBandMaxGridY = 65535;

int gqband_check(const char* who, int B, int H, int Hkv, int Lq, int Lk, int head_dim, int64_t q_rs, int64_t q_bs,
                 int64_t kv_rs, int64_t kv_bs, int start_pos, int window, uintptr_t ptr_or) {
  if (!gqband_hd_ok(head_dim)) {
    pdn_set_error("%s: head_dim %d not in {16, 24, 32, 48, 64, 96, 128}", who, head_dim);
    return PDN_EUNSUPPORTED;
  }
  if (!gqband_group_ok(H, Hkv)) {
    pdn_set_error("%s: %d query heads over %d key/value heads: the group size must be a whole number in 2 .. 8", who, H, Hkv);
    return PDN_EUNSUPPORTED;
  }
  if (window < 1) {
    pdn_set_error("%s: window %d: a query sees at least its own key", who, window);
    return PDN_EUNSUPPORTED;
  }
  if (start_pos < 0) {
    pdn_set_error("%s: start_pos %d is negative", who, start_pos);
    return PDN_EINVAL;
  }
  if ((int64_t)Lk < (int64_t)start_pos + Lq) {
    pdn_set_error("%s: Lk = %d keys for start_pos + Lq = %lld: every query must see its own key", who, Lk,
                  (long long)start_pos + Lq);
    return PDN_EUNSUPPORTED;
  }
  if ((int64_t)B * Hkv > kGqBandMaxGridY) {
    pdn_set_error("%s: B * Hkv = %lld exceeds the grid's y limit of %lld", who, (long long)B * Hkv,
                  (long long)kGqBandMaxGridY);
    return PDN_EUNSUPPORTED;
  }
  if ((q_rs % 4) || (q_bs % 4) || (kv_rs % 4) || (kv_bs % 4) || (ptr_or & 15)) {
    pdn_set_error("%s: 16-byte alignment of operands and strides required", who);
    return PDN_EINVAL;
  }
  return PDN_OK;
}

GqBandArgs gqband_args(int H, int Hkv, int Lq, int Lk, int head_dim, int64_t q_rs, int64_t q_bs, int64_t kv_rs,
                       int64_t kv_bs, int start_pos, int window) {
  // a window of start_pos + Lq or more is plain causal attention: clipped, so that no key index sum leaves int
  return GqBandArgs{{H, Lq, Lk, 1, start_pos, q_rs, q_bs, kv_rs, kv_bs, 1.f / sqrtf((float)head_dim), nullptr, 0, 0, 0, 0,
                     nullptr, nullptr},
                    window < start_pos + Lq ? window : start_pos + Lq, Hkv, H / Hkv};
}

dim3 gqband_unit_grid(int B, int H, int Hkv, int Lq) {
  const int64_t units = (int64_t)(H / Hkv) * ((Lq + 31) / 32);
  return dim3((unsigned)((units + 3) / 4), (unsigned)(B * Hkv));
}
}  // namespace

extern "C" {

int pdnm_attention_supported(int head_dim, int H, int Hkv) {
  return gqband_hd_ok(head_dim) && gqband_group_ok(H, Hkv) ? 1 : 0;
}

int64_t pdnm_attention_bwd_workspace_bytes(int B, int H, int Lq) { return 4ll * B * H * Lq; }

int pdnm_attention_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int Hkv,
                           int Lq, int Lk, int head_dim, int64_t q_row_stride, int64_t q_batch_stride,
                           int64_t kv_row_stride, int64_t kv_batch_stride, int start_pos, int window, void* stream) {
  if (B == 0 || H == 0 || Lq == 0) return PDN_OK;
  PDN_CHECK_ARG(q && k && v && o && lse && B > 0 && Lq > 0 && Lk > 0, "pdnm_attention_fwd_f32: bad operand");
  int rc = gqband_check("pdnm_attention_fwd_f32", B, H, Hkv, Lq, Lk, head_dim, q_row_stride, q_batch_stride, kv_row_stride,
                        kv_batch_stride, start_pos, window, (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o);
  if (rc) return rc;
  GqBandArgs ga = gqband_args(H, Hkv, Lq, Lk, head_dim, q_row_stride, q_batch_stride, kv_row_stride, kv_batch_stride,
                              start_pos, window);
  GQBAND_DISPATCH(head_dim, {
    auto kern = gqband_fwd_kernel<HD>;
    PDN_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gqband_lds(HD)));
    pdn_count(PDN_CNT_ATT_GQBAND);
    hipLaunchKernelGGL(kern, gqband_unit_grid(B, H, Hkv, Lq), dim3(256), gqband_lds(HD), (hipStream_t)stream, q, k, v, o,
                       lse, ga);
  });
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

int pdnm_attention_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                           const float* lse, float* dq, float* dk, float* dv, int B, int H, int Hkv, int Lq, int Lk,
                           int head_dim, int64_t q_row_stride, int64_t q_batch_stride, int64_t kv_row_stride,
                           int64_t kv_batch_stride, int start_pos, int window, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  if (B == 0 || H == 0 || Lq == 0) return PDN_OK;
  PDN_CHECK_ARG(q && k && v && o && d_o && lse && dq && dk && dv && B > 0 && Lq > 0 && Lk > 0,
                "pdnm_attention_bwd_f32: bad operand");
  int rc = gqband_check("pdnm_attention_bwd_f32", B, H, Hkv, Lq, Lk, head_dim, q_row_stride, q_batch_stride, kv_row_stride,
                        kv_batch_stride, start_pos, window,
                        (uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o | (uintptr_t)d_o | (uintptr_t)dq |
                            (uintptr_t)dk | (uintptr_t)dv);
  if (rc) return rc;
  if (!workspace || workspace_bytes < pdnm_attention_bwd_workspace_bytes(B, H, Lq)) {
    pdn_set_error("pdnm_attention_bwd_f32: workspace too small");
    return PDN_EWORKSPACE;
  }
  float* delta = (float*)workspace;
  GqBandArgs ga = gqband_args(H, Hkv, Lq, Lk, head_dim, q_row_stride, q_batch_stride, kv_row_stride, kv_batch_stride,
                              start_pos, window);
  hipStream_t st = (hipStream_t)stream;
  GQBAND_DISPATCH(head_dim, {
    auto kq = gqband_bwd_dq_kernel<HD>;
    auto kkv = gqband_bwd_dkv_kernel<HD>;
    PDN_HIP(hipFuncSetAttribute((const void*)kq, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gqband_lds(HD)));
    PDN_HIP(hipFuncSetAttribute((const void*)kkv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gqband_lds(HD)));
    pdn_count(PDN_CNT_ATT_GQBAND);
    hipLaunchKernelGGL(kq, gqband_unit_grid(B, H, Hkv, Lq), dim3(256), gqband_lds(HD), st, q, k, v, o, d_o, lse, dq, delta,
                       ga);
    hipLaunchKernelGGL(kkv, dim3((Lk + 127) / 128, B * Hkv), dim3(256), gqband_lds(HD), st, q, k, v, d_o, lse, delta, dk,
                       dv, ga);
  });
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

}  // extern "C"
