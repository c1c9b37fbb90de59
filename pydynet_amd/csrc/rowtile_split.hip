// q | k | v + RoPE, gate | up + SwiGLU and dh + SwiGLU backward on split-fp16 MFMA at fp32 accuracy (gfx950 only), for 16384
// rows and more:
//
//   qkv (M x 3D) = rmsnorm(x) [Wq | Wk | Wv], RoPE on the q and k blocks          (llm/llama/model.py:23-44, 93-104)
//   gu (M x 2F)  = rmsnorm(x) [Wg | Wu],  h = silu(gate) * up                     (model.py:56-58)
//   dgu (M x 2F) = SwiGLU'(gu) o (g2 W_down^T)                                    (model.py:56-58 backwards)
//
// the contracts of gemm_rowtile_kernel<false, 3 / 1, ., NORM> and <true, 2> (csrc/gemm_rowtile.hip), whose launch routes here
// (pdn_rowtile_launch: no entry of its own).  It is the product of csrc/lm_head_split.hip -- tall A, contraction exactly
// 288, A rows resident in registers as two fp16 planes, an N-sweep over 32-column tile images of W in a ring of three LDS
// slots, transposed accumulators (a lane owns a ROW), the finished tile leaving row-wise through a per-wave LDS area in the
// shadow of the next tile's MFMAs -- with two differences:
//   * no pass over x: the wave reads its 32 rows itself, ONCE and by whole 128-byte lines (eight lanes per row; 36
//     instructions, 144 registers).  From them it forms the sum of squares (the RMSNorm's) and the largest |x w| of each
//     row, from which the row's power of two follows (max |xn| = max |x w| / r up to round-off, which moves the planes'
//     top bit by at most one place).  Then, a chunk of 32 columns at a time, it normalises with the arithmetic of the fp32
//     kernel (x * (1 / r) * w), stores xn as whole lines, passes the 32 x 32 chunk through its staging area and reads it
//     back as the B fragments of two k-steps, which are split: 16 fp32 registers die as 16 plane registers are born, so
//     the 144 fp32 values and the 144 plane registers are never alive together.  Only the workgroups of the first column
//     range (blockIdx.y == 0) write xn / rms; with a null xn (include/pdn_normplanes.h) rms alone, under the same predicate.
//   * the epilogues run in the drain, AFTER the scale is removed (one ldexp with the sum of the two integer exponents):
//     RoPE rotates the pairs inside a lane's four columns with the table entries of its own row (the two EVEN columns'
//     entries serve both members of a pair), requested three or four slots ahead into four registers; SwiGLU meets
//     gate[c] in register i and up[c] in register i + 8 of the same lane, because a gate | up tile is 16 gate columns
//     followed by their 16 up columns (rowtile_split_index.h).  h is formed from
//     the still-scaled registers a second time (8 ldexp) rather than kept, and passes through the same LDS area once the
//     gu rows have left it.
//   * dh + SwiGLU backward (EPI 2): a tile is 32 dh columns = 32 rows of W_down (the W pass reads them along k).  Its
//     row-wise store step meets, per lane, the 16 bytes of gate and of up at its row and columns of gu and writes dgate
//     and dup there: whole 128-byte lines in all four streams.  The gu values of two row steps are held at a time (16
//     registers), requested behind the staging loads of the tile before or in front of those of slot 6 (run_tile).
// The tile images are built from the weights where they live; the optimiser changes them every step.  One small launch per
// call (rts_w_kernel) does it, unless the caller has bound a set that was built for the whole pass in one launch
// (include/pdn_wimages.h) and holds this weight in this form.  Every address comes from rowtile_split_index.h, which
// tests/rowtile_split_check.cpp walks on the host.
// Deterministic: fixed order, no atomics.
#include "common.h"
#include "lm_head_split.h"
#include "gemm_rowtile.h"
#include "rowtile_split_index.h"
#include "weight_images.h"
#include <stdlib.h>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

extern "C" int pdn_malloc(void** ptr, int64_t bytes);
extern "C" int pdn_free(void* ptr);

// ---- W: one workgroup per tile (the body: csrc/weight_images.h, shared with the batched builder) -------------------------
__global__ __launch_bounds__(256) void rts_w_kernel(RtsWParams p) {
  __shared__ float sm[RTS_W_SM];
  __shared__ float smax[RTS_W_SMAX];
  rts_w_tile(p, blockIdx.x, sm, smax);
}

// ---- the product ------------------------------------------------------------------------------------------------
struct RtsParams {
  const float* A;
  int64_t lda;
  const char* wimg;
  float* C;
  float* H;
  const float* GU;                // EPI 2: the saved [gate | up] rows, leading dimension ldc
  unsigned ldc, ldh;
  const float* rope;
  int L, hd, rope_tiles;
  unsigned hd_magic;              // ceil(2^32 / hd)
  int F;
  const float* norm_w;
  float* xn;
  float* rms;
  int64_t ldxn;
  float norm_eps;
  int M, ntiles, tpw;
  int ablate;                     // PDN_ROWTILE_SPLIT_ABLATE (timing experiments; 0 in the library): 1 = no stores,
                                  // 2 = constant planes (the rows of x are not read), 4 = EPI 2: the gu rows are not read
};

template <int V> using rts_ic = std::integral_constant<int, V>;

__device__ __forceinline__ float rts_sigmoid(float g) {     // rt_sigmoid of csrc/gemm_rowtile.hip
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * g));
}

// EPI: 1 SwiGLU, 2 SwiGLU backward (W transposed, NORM never), 3 RoPE.  GUARD: M is not a multiple of 256 (row test in every store).  NORM: A holds the rows BEFORE
// the RMSNorm.  LDS: the ring of three tile images and the eight staging areas of ls_main_kernel.
template <int EPI, bool GUARD, bool NORM>
__global__ __launch_bounds__(512, 1) void rts_main_kernel(RtsParams p) {
  static_assert(EPI == 1 || EPI == 2 || EPI == 3, "SwiGLU, SwiGLU backward or RoPE");
  static_assert(EPI != 2 || !NORM, "SwiGLU backward: no RMSNorm in front");
  __shared__ __attribute__((aligned(16))) char smem[RTS_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int m0 = (blockIdx.x * 8 + wave) * 32;
  const int T0 = blockIdx.y * p.tpw;
  const int T1 = min(p.ntiles, T0 + p.tpw);
  if (T0 >= T1) return;                             // (the whole workgroup)

  const bool q4_on = rts_stage_on(4, tid);
  auto stage_ld = [&](const char* base, int q, uint4& r) __attribute__((always_inline)) {
    if (q < 4 || q4_on) r = *reinterpret_cast<const uint4*>(base + (unsigned)rts_stage_unit(q, tid) * 16u);
  };
  auto stage_park = [&](int slot, int q, const uint4& r) __attribute__((always_inline)) {
    if (q < 4 || q4_on) *reinterpret_cast<uint4*>(smem + slot + rts_stage_unit(q, tid) * 16) = r;
  };

  // ---- prologue: the first tile into slot 0 ------------------------------------------------------------------------
  {
    const char* b0 = p.wimg + (int64_t)T0 * RTS_TILE;
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0, t2 = t0, t3 = t0, t4 = t0;
    stage_ld(b0, 0, t0); stage_ld(b0, 1, t1); stage_ld(b0, 2, t2); stage_ld(b0, 3, t3); stage_ld(b0, 4, t4);
    stage_park(0, 0, t0); stage_park(0, 1, t1); stage_park(0, 2, t2); stage_park(0, 3, t3); stage_park(0, 4, t4);
  }
  // ---- the wave's 32 rows: statistics, then normalise / store / split ------------------------------------------------
  char* stg0 = smem + 3 * RTS_TILE + wave * RTS_STG;
  f16x8 xh[RTS_KS], xl[RTS_KS];
  int nexv = 0;
  if (p.ablate & 2) {
#pragma unroll
    for (int s = 0; s < RTS_KS; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) { xh[s][j] = (_Float16)1.f; xl[s][j] = (_Float16)0.5f; }
  } else {
    // whole 128-byte lines: instruction (c, i) takes columns 32 c + 4 (lane & 7) .. + 3 of row 8 i + (lane >> 3), eight
    // lanes per row and line; every element of the 32 rows is read ONCE and stays in registers until its chunk is split
    const char* arow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      arow[i] = reinterpret_cast<const char*>(p.A + rts_a_row(m0, rts_pl_row(lane, i), p.M) * p.lda + rts_pl_col(lane, 0));
    const char* wp = reinterpret_cast<const char*>(p.norm_w + rts_pl_col(lane, 0));
    float4 xa[RTS_CHUNKS][4];
#pragma unroll
    for (int c = 0; c < RTS_CHUNKS; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) xa[c][i] = *reinterpret_cast<const float4*>(arow[i] + 128 * c);
    // statistics of the lane's four rows: sum of squares, max |x w| (INFINITY once an Inf or NaN was seen: fmaxf alone
    // would drop a NaN, the sum of the four does not)
    float ss[4] = {0.f, 0.f, 0.f, 0.f}, am[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < RTS_CHUNKS; ++c) {
      float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
      if (NORM) w = *reinterpret_cast<const float4*>(wp + 128 * c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 a = xa[c][i];
        ss[i] += (a.x * a.x + a.y * a.y) + (a.z * a.z + a.w * a.w);
        const float f0 = fabsf(a.x * w.x), f1 = fabsf(a.y * w.y), f2 = fabsf(a.z * w.z), f3 = fabsf(a.w * w.w);
        am[i] = fmaxf(am[i], fmaxf(fmaxf(f0, f1), fmaxf(f2, f3)));
        if (!((f0 + f1) + (f2 + f3) < INFINITY)) am[i] = INFINITY;
      }
    }
    // the eight lanes of a row, in a fixed order; then every one of them has the row's r, 1 / r and shift
    float inv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int d = 1; d < 8; d <<= 1) {
        ss[i] += __shfl_xor(ss[i], d, 64);
        am[i] = fmaxf(am[i], __shfl_xor(am[i], d, 64));
      }
      float r = 1.f;
      inv[i] = 1.f;
      if (NORM) { r = sqrtf(ss[i] / 288.f + p.norm_eps); inv[i] = 1.f / r; }
      const float amax = NORM ? am[i] * inv[i] : am[i];
      const int sh_i = ls_shift(!(amax < INFINITY) ? INFINITY : amax);      // a non-finite row keeps scale 1 and comes out NaN
      // to the lanes that own the row's fragments, through the wave's staging area (free before the first tile leaves)
      if ((lane & 7) == 0)
        *reinterpret_cast<float2*>(__builtin_assume_aligned(stg0 + rts_pl_stat(rts_pl_row(lane, i)), 8)) = make_float2(r, __int_as_float(sh_i));
    }
    const float2 st = *reinterpret_cast<const float2*>(__builtin_assume_aligned(stg0 + rts_pl_stat(li), 8));
    const int sh = __float_as_int(st.y);
    nexv = -sh;
    const bool wr_on = blockIdx.y == 0 && !(p.ablate & 1);
    if (NORM && lh == 0 && wr_on && (!GUARD || m0 + li < p.M)) p.rms[m0 + li] = st.x;
    const bool xn_on = wr_on && p.xn != nullptr;    // (no xn: the caller's backward works from x, norm_w and rms)
    char* xrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      xrow[i] = reinterpret_cast<char*>(p.xn + rts_a_row(m0, rts_pl_row(lane, i), p.M) * p.ldxn + rts_pl_col(lane, 0));
    char* pw = stg0 + rts_pl_stg_w(lane, 0);        // row step i: 8 i rows further on
    const char* pf = stg0 + rts_pl_stg_r(li, lh, 0, 0);
    // a chunk of 32 columns (two k-steps): normalise where it was loaded, xn leaves as whole lines, the 32 x 32 chunk
    // passes through the staging area (row pitch 144) and comes back as the B fragments k = 16 s + 8 lh .. + 7 of row li
#pragma unroll
    for (int c = 0; c < RTS_CHUNKS; ++c) {
      float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
      if (NORM) w = *reinterpret_cast<const float4*>(wp + 128 * c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float4 v = xa[c][i];
        if (NORM) {
          v.x = v.x * inv[i] * w.x; v.y = v.y * inv[i] * w.y; v.z = v.z * inv[i] * w.z; v.w = v.w * inv[i] * w.w;
          if (xn_on && (!GUARD || m0 + rts_pl_row(lane, i) < p.M)) *reinterpret_cast<float4*>(xrow[i] + 128 * c) = v;
        }
        *reinterpret_cast<float4*>(__builtin_assume_aligned(pw + i * (8 * 144), 16)) = v;
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int s = 2 * c + e;
        const float4 va = *reinterpret_cast<const float4*>(__builtin_assume_aligned(pf + 64 * e, 16));
        const float4 vb = *reinterpret_cast<const float4*>(__builtin_assume_aligned(pf + 64 * e + 16, 16));
        const float v[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          _Float16 h, l;
          ls_split(v[j], sh, h, l);
          xh[s][j] = h; xl[s][j] = l;
        }
      }
    }
  }

  f32x16 acc0, acc1;
  float out[16];                                    // the tile that leaves: acc0 + acc1 / 2048, still scaled
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; out[r] = 0.f; }
  const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  const int fr_even = rts_frag_base(li, lh, 0), fr_odd = rts_frag_base(li, lh, 1);
  const int tail_lane = RTS_TAIL + 4 * rts_reg_col(0, lh);   // group g: 32 g bytes further on
  char* stg = stg0;
  char* stg_w = stg + rts_stg_w(li, lh, 0);         // group g: 32 g bytes further on
  const char* stg_r = stg + rts_stg_r(lane, 0);     // store j: 8 j rows further on
  const char* stgh_r = stg + rts_h_r(lane, 0);      // h store j: 16 j rows further on
  const bool st_all = !(p.ablate & 1);
  const int srow = m0 + rts_st_row(lane, 0), hrow = m0 + rts_h_row(lane, 0);
  // BYTES beside a wave-uniform base (the tile's first column); gate | up: the up half of a row lies 4 F bytes after the gate half
  const unsigned ob = 4u * (unsigned)rts_st_row(lane, 0) * p.ldc +
                      (EPI == 1 ? ((lane & 4) ? 4u * (unsigned)p.F + 16u * (unsigned)(lane & 3) : 16u * (unsigned)(lane & 3))
                                : 4u * (unsigned)rts_st_col(lane));
  const unsigned obh = 4u * (unsigned)rts_h_row(lane, 0) * p.ldh + 16u * (unsigned)(lane & 3);
  const unsigned ldc32 = 32u * p.ldc, ldh64 = 64u * p.ldh;   // eight rows of C / sixteen rows of H, in bytes
  const unsigned Fb = 4u * (unsigned)p.F;           // EPI 2: dup / up lie F floats after dgate / gate
  const bool gu_on = !(p.ablate & 4);
  // EPI 2: the saved gate / up values of two row steps (rows 8 j + (lane >> 3), columns 4 (lane & 7) .. + 3 of the tile)
  float4 pg[2], pu[2];
  pg[0] = pg[1] = pu[0] = pu[1] = make_float4(1.f, 1.f, 1.f, 1.f);
  const unsigned tab_lane = 8u * (unsigned)rts_rope_pos(m0, li, p.L) * (unsigned)p.hd;   // this lane's row of the table, in bytes

  // the table entries of the two even columns of group g of tile t: (cos, -sin, cos', -sin')
  auto rope_ld = [&](int t, int g, float4& r) __attribute__((always_inline)) {
    const unsigned x = 32u * (unsigned)t + 8u * (unsigned)g + 4u * (unsigned)lh;
    const unsigned colh = rts_rope_colh_magic(x, (unsigned)p.hd, p.hd_magic);
    const char* src = reinterpret_cast<const char*>(p.rope) + (tab_lane + 8u * colh);
    const float2 a = *reinterpret_cast<const float2*>(src), b = *reinterpret_cast<const float2*>(src + 16);
    r.x = a.x; r.y = a.y; r.z = b.x; r.w = b.y;
  };
  // group g (registers 4 g .. 4 g + 3 = tile columns 8 g + 4 lh .. + 3) of the leaving tile: scale removed, then RoPE
  auto drain_group = [&](int g, const int4& ne, const float4& tb, bool rot) __attribute__((always_inline)) {
    float4 o;
    o.x = ldexpf(out[4 * g + 0], nexv + ne.x);
    o.y = ldexpf(out[4 * g + 1], nexv + ne.y);
    o.z = ldexpf(out[4 * g + 2], nexv + ne.z);
    o.w = ldexpf(out[4 * g + 3], nexv + ne.w);
    if (EPI == 3) {
      // out = v cos + pair(v) * (column odd ? sin : -sin), as the fp32 kernel forms it
      const float ex = fmaf(o.x, tb.x, o.y * tb.y), oy = fmaf(o.y, tb.x, -(o.x * tb.y));
      const float ez = fmaf(o.z, tb.z, o.w * tb.w), ow = fmaf(o.w, tb.z, -(o.z * tb.w));
      if (rot) { o.x = ex; o.y = oy; o.z = ez; o.w = ow; }
    }
    *reinterpret_cast<float4*>(__builtin_assume_aligned(stg_w + 32 * g, 16)) = o;
  };
  // h columns 8 g + 4 lh .. + 3 of the leaving gate | up tile (g = 0, 1): ng / nu = the exponents of its gate / up columns
  auto h_group = [&](int g, const int4& ng, const int4& nu) __attribute__((always_inline)) {
    const float g0 = ldexpf(out[4 * g + 0], nexv + ng.x), u0 = ldexpf(out[4 * g + 8], nexv + nu.x);
    const float g1 = ldexpf(out[4 * g + 1], nexv + ng.y), u1 = ldexpf(out[4 * g + 9], nexv + nu.y);
    const float g2 = ldexpf(out[4 * g + 2], nexv + ng.z), u2 = ldexpf(out[4 * g + 10], nexv + nu.z);
    const float g3 = ldexpf(out[4 * g + 3], nexv + ng.w), u3 = ldexpf(out[4 * g + 11], nexv + nu.w);
    float4 o;
    o.x = g0 * rts_sigmoid(g0) * u0; o.y = g1 * rts_sigmoid(g1) * u1;
    o.z = g2 * rts_sigmoid(g2) * u2; o.w = g3 * rts_sigmoid(g3) * u3;
    *reinterpret_cast<float4*>(__builtin_assume_aligned(stg + rts_h_w(li, lh, 0) + 32 * g, 16)) = o;
  };
  // store j: rows 8 j .. 8 j + 7 of the tile, a 128-byte line (gate | up: two 64-byte segments) per eight lanes
  auto store_rows = [&](int j, float* Cd) __attribute__((always_inline)) {
    const float4 v = *reinterpret_cast<const float4*>(__builtin_assume_aligned(stg_r + j * (8 * 144), 16));
    if (st_all && (!GUARD || srow + 8 * j < p.M))
      *reinterpret_cast<float4*>(reinterpret_cast<char*>(Cd) + ob + (unsigned)j * ldc32) = v;
  };
  // h store j: rows 16 j .. 16 j + 15, a 64-byte segment per four lanes
  auto store_h = [&](int j, float* Hd) __attribute__((always_inline)) {
    const float4 v = *reinterpret_cast<const float4*>(__builtin_assume_aligned(stgh_r + j * (16 * 144), 16));
    if (st_all && (!GUARD || hrow + 16 * j < p.M))
      *reinterpret_cast<float4*>(reinterpret_cast<char*>(Hd) + obh + (unsigned)j * ldh64) = v;
  };
  // EPI 2: gate and up of row step j of the tile whose first gate column is at Gd: a whole 128-byte line per eight lanes each
  auto gu_ld = [&](int j, const float* Gd, float4& g, float4& u) __attribute__((always_inline)) {
    if (gu_on && (!GUARD || srow + 8 * j < p.M)) {
      const char* src = reinterpret_cast<const char*>(Gd) + ob + (unsigned)j * ldc32;
      g = *reinterpret_cast<const float4*>(src);
      u = *reinterpret_cast<const float4*>(src + Fb);
    }
  };
  // EPI 2 store j: dh of rows 8 j .. 8 j + 7 from the staging area, the arithmetic of gemm_rowtile_kernel<., 2>
  auto store_bwd = [&](int j, float* Cd, const float4& g, const float4& u) __attribute__((always_inline)) {
    const float4 d = *reinterpret_cast<const float4*>(__builtin_assume_aligned(stg_r + j * (8 * 144), 16));
    const float dh[4] = {d.x, d.y, d.z, d.w}, gv[4] = {g.x, g.y, g.z, g.w}, uv[4] = {u.x, u.y, u.z, u.w};
    float dg[4], du[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = rts_sigmoid(gv[i]), sl = gv[i] * s;
      const float dsl = fmaf(sl, 1.f - s, s);       // silu'(g) = s (1 + g (1 - s))
      dg[i] = dh[i] * uv[i] * dsl; du[i] = dh[i] * sl;
    }
    if (st_all && (!GUARD || srow + 8 * j < p.M)) {
      char* dst = reinterpret_cast<char*>(Cd) + ob + (unsigned)j * ldc32;
      *reinterpret_cast<float4*>(dst) = make_float4(dg[0], dg[1], dg[2], dg[3]);
      *reinterpret_cast<float4*>(dst + Fb) = make_float4(du[0], du[1], du[2], du[3]);
    }
  };
  auto g_of = [&](int t) -> const float* { return p.GU + (int64_t)m0 * p.ldc + 32 * t; };
  auto c_of = [&](int t) -> float* { return p.C + (int64_t)m0 * p.ldc + (EPI == 1 ? 16 : 32) * t; };
  auto h_of = [&](int t) -> float* { return p.H + (int64_t)m0 * p.ldh + 16 * t; };

  // ---- one tile: 18 k-steps of 3 MFMAs out of slot `cur`; in their shadow tile t + 1 is staged into `nxt` (two
  // instructions in flight: requested in slots 0, 6, 12, parked in 6, 12, 17) and tile t - 1 leaves (its exponents: slot
  // `prv`).  vmcnt retires in order, so every request is placed BEFORE the staging loads that may still be on their way
  // when it is needed.  Slots of the leaving tile:
  //   RoPE:   the table entries of group g are requested in slots 0, 4, 8, 12 (four registers) and the group is drained
  //           in 4, 8, 12, 15; row stores in 16, 17
  //   SwiGLU: groups drained in 1, 3, 5, 7; gu row stores in 8 .. 11; h formed in 12, 13 and stored in 14, 15
  //   SwiGLU backward: groups drained in 0 .. 3; row steps 0, 1 leave in 4, 5 with the gate / up values requested in slot
  //           13 of the tile BEFORE (behind that tile's last staging load, long arrived); the values of row steps 2, 3 are
  //           requested in slot 6 into the same registers, in front of the staging loads of that slot, and used in 11, 12
  auto run_tile = [&](auto firstc, int t, int cur, int prv, int nxt) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(firstc)::value != 0;
    lds_barrier();
    const char* nb = p.wimg + (int64_t)min(t + 1, T1 - 1) * RTS_TILE;   // (after the last tile: a redundant fetch into an idle slot)
    float* Cd = c_of(t - 1);
    float* Hd = EPI == 1 ? h_of(t - 1) : nullptr;
    const bool rot = EPI == 3 && t - 1 < p.rope_tiles;
    const char* fe = smem + cur + fr_even;
    const char* fo = smem + cur + fr_odd;
    const char* tl = smem + prv + tail_lane;
    f16x8 wh[2], wl;
    uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
    int4 ne = make_int4(0, 0, 0, 0), nu = ne;
    float4 tb = make_float4(0.f, 0.f, 0.f, 0.f);
#define RTS_LOADH(X, S) wh[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned((((S) & 1) ? fo : fe) + rts_frag_step(S), 16));
#define RTS_LOADL(S) wl = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned((((S) & 1) ? fo : fe) + rts_frag_step(S) + RTS_PLANE, 16));
    RTS_LOADH(0, 0)
    RTS_LOADL(0)
#pragma unroll
    for (int s = 0; s < RTS_KS; ++s) {
      if (s + 1 < RTS_KS) { RTS_LOADH((s + 1) & 1, s + 1) }
      // which group leaves for the LDS area in this slot (-1: none), and which h group is formed
      const int dg = EPI == 1 ? (((s & 1) && s < 8) ? (s >> 1) : -1)
                     : EPI == 2 ? (s < 4 ? s : -1)
                              : (s == 4 ? 0 : s == 8 ? 1 : s == 12 ? 2 : s == 15 ? 3 : -1);
      const int hg = EPI == 1 ? (s == 12 ? 0 : s == 13 ? 1 : -1) : -1;
      if (!FIRST && dg >= 0) ne = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl + 32 * dg, 16));
      if (!FIRST && hg >= 0) {
        ne = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl + 32 * hg, 16));
        nu = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl + 32 * hg + 64, 16));
      }
      __builtin_amdgcn_sched_barrier(0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[s & 1], xh[s], s == 0 ? zero16 : acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh[s], s == 0 ? zero16 : acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // (the l plane is single-buffered: its registers are free once the MFMA above has been issued)
      if (s + 1 < RTS_KS) { RTS_LOADL(s + 1) }
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[s & 1], xl[s], acc1, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // ---- slot s ----
      if (s == 6) { stage_park(nxt, 0, r0); stage_park(nxt, 1, r1); }
      if (s == 12) { stage_park(nxt, 2, r0); stage_park(nxt, 3, r1); }
      if (s == 17) stage_park(nxt, 4, r0);
      if (!FIRST && dg >= 0) drain_group(dg, ne, tb, rot);
      if (EPI == 3 && !FIRST && (s == 0 || s == 4 || s == 8 || s == 12)) rope_ld(t - 1, s >> 2, tb);
      if (EPI == 2 && !FIRST && (s == 4 || s == 5)) store_bwd(s - 4, Cd, pg[s - 4], pu[s - 4]);
      if (EPI == 2 && !FIRST && s == 6) { gu_ld(2, g_of(t - 1), pg[0], pu[0]); gu_ld(3, g_of(t - 1), pg[1], pu[1]); }
      if (EPI == 2 && !FIRST && (s == 11 || s == 12)) store_bwd(s - 9, Cd, pg[s - 11], pu[s - 11]);
      if (s == 0) { stage_ld(nb, 0, r0); stage_ld(nb, 1, r1); }
      if (s == 6) { stage_ld(nb, 2, r0); stage_ld(nb, 3, r1); }
      if (s == 12) stage_ld(nb, 4, r0);
      if (EPI == 2 && s == 13) { gu_ld(0, g_of(t), pg[0], pu[0]); gu_ld(1, g_of(t), pg[1], pu[1]); }   // of THIS tile: it leaves next
      if (EPI == 3 && !FIRST && s >= 16) { store_rows(2 * (s - 16), Cd); store_rows(2 * (s - 16) + 1, Cd); }
      if (EPI == 1 && !FIRST && s >= 8 && s < 12) store_rows(s - 8, Cd);
      if (!FIRST && hg >= 0) h_group(hg, ne, nu);
      if (EPI == 1 && !FIRST && (s == 14 || s == 15)) store_h(s - 14, Hd);
      __builtin_amdgcn_sched_barrier(0);
    }
#undef RTS_LOADH
#undef RTS_LOADL
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = fmaf(acc1[r], 1.f / 2048.f, acc0[r]);
  };

  int cur = 0, prv = 2 * RTS_TILE, nxt = RTS_TILE;
  run_tile(rts_ic<1>{}, T0, cur, prv, nxt);
  for (int t = T0 + 1; t < T1; ++t) {
    prv = cur; cur = nxt; nxt = nxt == 2 * RTS_TILE ? 0 : nxt + RTS_TILE;
    run_tile(rts_ic<0>{}, t, cur, prv, nxt);
  }
  // the last tile leaves with nothing to hide behind (its slot is not written again)
  {
    float* Cd = c_of(T1 - 1);
    const bool rot = EPI == 3 && T1 - 1 < p.rope_tiles;
    const char* tl = smem + cur + tail_lane;
    float4 tb[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      tb[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (EPI == 3) rope_ld(T1 - 1, g, tb[g]);
    }
    float4 lg[2], lu[2];                            // EPI 2: row steps 2, 3 (0, 1 were requested in slot 13)
    lg[0] = lg[1] = lu[0] = lu[1] = make_float4(1.f, 1.f, 1.f, 1.f);
    if (EPI == 2) { gu_ld(2, g_of(T1 - 1), lg[0], lu[0]); gu_ld(3, g_of(T1 - 1), lg[1], lu[1]); }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int4 ne = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl + 32 * g, 16));
      drain_group(g, ne, tb[g], rot);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (EPI == 2) {
      store_bwd(0, Cd, pg[0], pu[0]); store_bwd(1, Cd, pg[1], pu[1]);
      store_bwd(2, Cd, lg[0], lu[0]); store_bwd(3, Cd, lg[1], lu[1]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) store_rows(j, Cd);
    }
    if (EPI == 1) {
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int4 ng = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl + 32 * g, 16));
        const int4 nu = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl + 32 * g + 64, 16));
        h_group(g, ng, nu);
      }
      __builtin_amdgcn_sched_barrier(0);
      float* Hd = h_of(T1 - 1);
      store_h(0, Hd); store_h(1, Hd);
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// Scratch from the library's allocator, with the two-stream rule of AbTemp (csrc/attention_blocks.hip): the pool orders
// reuse on the compute stream only, so with the opt-in second stream the free waits for our kernels first.
namespace {
struct RtsTemp {
  void* p = nullptr;
  hipStream_t st = nullptr;
  int get(int64_t bytes, void* stream) { st = (hipStream_t)stream; return pdn_malloc(&p, bytes); }
  ~RtsTemp() {
    static const bool two_stream = getenv("PDN_TWO_STREAM") && atoi(getenv("PDN_TWO_STREAM")) != 0;
    if (p && two_stream) (void)hipStreamSynchronize(st);
    if (p) pdn_free(p);
  }
};
}

static int rts_tiles(const RowTileArgs& a) { return a.epi == 1 ? a.F / 16 : a.N / 32; }

// PDN_ROWTILE_SPLIT=0: the fp32 kernel at every size (A/B switch; read once, announced)
int pdn_rowtile_split_enabled() {
  static const int s_on = ls_env_switch("PDN_ROWTILE_SPLIT", 1, "the q | k | v and gate | up projections and dh + SwiGLU backward stay on the fp32 MFMA kernel");
  return s_on;
}
int pdn_rowtile_split_takes(const RowTileArgs& a, void* stream) {
  if (!pdn_rowtile_split_enabled() ||(a.epi != 1 && a.epi != 2 && a.epi != 3) || a.M < RTS_MIN_ROWS || a.bias || a.residual) return 0;
  if ((a.epi == 2) != (a.b_trans != 0)) return 0;
  if (a.N < 32 || a.N % 32 != 0 || a.nblocks < 1 || (a.N / a.nblocks) * a.nblocks != a.N || (a.N / a.nblocks) % 32 != 0) return 0;
  if ((a.lda & 3) || (a.ldc & 3) || a.lda < RTS_K || a.ldc < a.N || a.ldc >= (1 << 24) || a.ldb < (a.b_trans ? RTS_K : a.N / a.nblocks)) return 0;
  if (((uintptr_t)a.A | (uintptr_t)a.C) & 15) return 0;
  if (a.epi == 1 && (a.F < 16 || a.F % 16 != 0 || a.N != 2 * a.F || a.nblocks != 2 || !a.H || (a.ldh & 3) || a.ldh < a.F ||
                     a.ldh >= (1 << 24) || ((uintptr_t)a.H & 15)))
    return 0;
  if (a.epi == 2) {
    // dgu (M x 2F) = SwiGLU'(gu) o (A W_down^T): W_down (F x 288) row-major, gu and dgu packed [gate | up] with ldc; an
    // in-place caller (C over GU) never comes here (gemm_rowres.hip), and this kernel reads gu rows after it wrote others
    if (a.F < 32 || a.F % 32 != 0 || a.N != a.F || a.nblocks != 1 || a.ldc < 2 * (int64_t)a.F || !a.GU || ((uintptr_t)a.GU & 15)) return 0;
    const float* ce = a.C + (int64_t)a.M * a.ldc;
    if ((const float*)a.C < a.GU + (int64_t)a.M * a.ldc && a.GU < ce) return 0;
    if ((const float*)a.C < a.A + (int64_t)a.M * a.lda && a.A < ce) return 0;
  }
  if (a.epi == 3 && (!a.rope || a.hd < 4 || a.hd % 4 != 0 || a.L < 1 || a.rope_cols % 32 != 0 || a.rope_cols > a.N ||
                     (int64_t)a.L * a.hd >= (1 << 27) || ((uintptr_t)a.rope & 7)))
    return 0;
  // (xn may be null: rms alone is left for the backward)
  if (a.norm_w && !(a.rms && (!a.xn || ((a.ldxn & 3) == 0 && a.ldxn >= RTS_K)) && (((uintptr_t)a.xn | (uintptr_t)a.norm_w) & 15) == 0)) return 0;
  // the W images come from the library's allocator, which a stream that is being captured must not call
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return cs == hipStreamCaptureStatusNone ? 1 : 0;
}

int pdn_rowtile_split_launch(const RowTileArgs& a, void* stream) {
  static const int s_ablate = ls_env_switch("PDN_ROWTILE_SPLIT_ABLATE", 0, "timing ablation active, the results of the split q | k | v, gate | up and dh + SwiGLU backward kernels are WRONG");
  const int nt = rts_tiles(a);
  hipStream_t st = (hipStream_t)stream;
  // the image: from the set bound to this thread when it holds exactly this weight in this form (csrc/weight_images.hip),
  // else built here
  const PdnwDesc key = pdnw_key_rts(a.epi, a.B, a.N, a.nblocks, a.ldb, a.b_block_stride, a.g_off, a.u_off, a.F);
  RtsWParams w = rts_w_params(key);
  RtsTemp img;
  if (!pdnw_lookup(key, stream, &w.wimg, nullptr)) {
    const int rc = img.get((int64_t)nt * RTS_TILE, stream);
    if (rc) return rc;
    w.wimg = static_cast<char*>(img.p);
    hipLaunchKernelGGL(rts_w_kernel, dim3(nt), dim3(256), 0, st, w);
  }
  RtsParams p;
  memset(&p, 0, sizeof(p));
  p.A = a.A; p.lda = a.lda; p.wimg = w.wimg; p.C = a.C; p.H = a.H; p.GU = a.GU ? a.GU : a.A; p.ldc = (unsigned)a.ldc; p.ldh = (unsigned)a.ldh;
  p.rope = a.rope ? a.rope : a.A; p.L = a.L > 0 ? a.L : 1; p.hd = a.hd > 0 ? a.hd : 32; p.rope_tiles = a.rope_cols / 32;
  p.hd_magic = rts_rope_magic(p.hd);
  p.F = a.F; p.norm_w = a.norm_w ? a.norm_w : a.A; p.xn = a.norm_w ? a.xn : a.C; p.rms = a.rms; p.ldxn = a.ldxn; p.norm_eps = a.norm_eps;
  p.M = a.M; p.ntiles = nt; p.ablate = s_ablate;
  int parts;
  rts_plan(a.M, nt, &p.tpw, &parts);
  const dim3 grid((a.M + 255) / 256, parts), block(512);
  const bool guard = a.M % 256 != 0, norm = a.norm_w != nullptr;
#define RTS_LAUNCH(EPI_)                                                                                      \
  if (guard) { if (norm) hipLaunchKernelGGL((rts_main_kernel<EPI_, true, true>), grid, block, 0, st, p);      \
               else hipLaunchKernelGGL((rts_main_kernel<EPI_, true, false>), grid, block, 0, st, p); }        \
  else { if (norm) hipLaunchKernelGGL((rts_main_kernel<EPI_, false, true>), grid, block, 0, st, p);           \
         else hipLaunchKernelGGL((rts_main_kernel<EPI_, false, false>), grid, block, 0, st, p); }
  if (a.epi == 1) { RTS_LAUNCH(1) }
  else if (a.epi == 3) { RTS_LAUNCH(3) }
  else if (guard) hipLaunchKernelGGL((rts_main_kernel<2, true, false>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((rts_main_kernel<2, false, false>), grid, block, 0, st, p);
#undef RTS_LAUNCH
  // slots 2 / 4 as well: "gate | up + SwiGLU" and "q | k | v + RoPE" on the tile kernel are what bench.py's path check asks
  // for, whichever pipe ran them
  // (dh + SwiGLU backward: slot 3, and its own slot 51 rather than 41)
  pdn_count(PDN_CNT_ROWTILE_PLAIN + a.epi);
  pdn_count(a.epi == 2 ? PDN_CNT_ROWTILE_BWD_SPLIT : PDN_CNT_ROWTILE_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
