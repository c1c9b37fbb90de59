// The packed layer weight gradients on split-fp16 MFMA at fp32 accuracy (gfx950 only):
//
//   dW_b[d][c] = sum_t x[t][d] g[t][b * nb_cols + c]      x^T (288 x K) against dq | dk | dv (K x 864, three blocks of
//                                                         288 columns) or dgate | dup (K x 1536, two blocks of 768)
//
// the product of gemm_outres_tn_kernel<8, false, true> behind pdn_gemm_outres_tn_blocks_launch (csrc/gemm_outres.hip;
// `A^T @ grad` of pydynet/core/tensor.py:672-675), routed here by the packed-blocks branch of pdn_gemm_f32 (csrc/gemm.hip)
// from 32768 tokens on.  Both operands are fp16 planes, as in the lm_head weight gradient (csrc/lm_head_dw_split.hip), whose
// structure this is: a wave owns SIXTEEN columns of g and all 288 rows of dW of them on `v_mfma_f32_16x16x32_f16` (18 tiles
// x 4 registers x 2 sums), eight waves = 128 columns per workgroup, K cut into ranges over grid.y whose slabs the
// gemm_splitk_reduce_kernel launch of the caller combines (with beta).
//
//   x[:, d] 2^s(d) = xh + xl / 2048     three passes per call: column maxima, exponents, plane images in LDS order
//   g 2^S = gh + gl / 2048              formed in registers from raw fp32 g, which is read exactly ONCE by LDS-DMA into a
//                                       swizzled ring of four pieces and read back transposed between the MFMAs
//   dW 2^(S + s(d)) = xh gh + (xh gl + xl gh) / 2048
//
// S is a RUNNING exponent, one per wave: g has no bound like the |g| <= 1 of the cross-entropy gradient, and a pass over its
// 453 / 805 MB to find one would cost what the kernel saves.  Before a wave splits the 32 x 16 values of the next piece it
// takes the largest finite magnitude among them (lane maximum over eight values, DPP within rows of 16, four readlanes).
// If that times 2^S would reach 2^15 it picks the S that puts it into [2^12, 2^13), splits with the new S, and once the
// current piece's MFMAs are issued multiplies both accumulator sets by the exact power of two between the old and the new
// S: a wave-uniform branch taken once per three octaves of growth.  S starts from the first non-zero piece and only ever
// falls; an all-zero piece changes nothing; non-finite values are left out of the maximum and come out NaN in their column.
//
// Everything the loop fetches arrives by LDS-DMA (see csrc/lm_head_dw_split.hip for the order of the waits); every address
// comes from outres_tn_split_index.h, which tests/outres_tn_split_check.cpp walks on the host.  Deterministic: fixed order,
// no atomics.
#include "common.h"
#include "lm_head_split.h"
#include "outres_tn_split_index.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- X: column maxima over a range of rows (partial), then the exponent of every column ------------------------------
// 288 threads: thread (c4 = tid % 72, g = tid / 72) takes the float4 c4 of rows g, g + 4, .. of the block's range
__global__ __launch_bounds__(288) void ots_x_colmax_kernel(const float* __restrict__ x, int64_t ldx, int rows, int rows_per_block,
                                                            float* __restrict__ partial) {
  __shared__ float sm[4][LDW_N];
  const int c4 = threadIdx.x % 72, g = threadIdx.x / 72;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 z = m;                 // fmaxf drops a NaN: 0 * v stays 0 for every finite v and turns NaN for Inf and NaN
#pragma unroll 4
  for (int r = r0 + g; r < r1; r += 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + (int64_t)r * ldx + 4 * c4);
    m.x = fmaxf(m.x, fabsf(v.x)); m.y = fmaxf(m.y, fabsf(v.y)); m.z = fmaxf(m.z, fabsf(v.z)); m.w = fmaxf(m.w, fabsf(v.w));
    z.x = fmaf(v.x, 0.f, z.x); z.y = fmaf(v.y, 0.f, z.y); z.z = fmaf(v.z, 0.f, z.z); z.w = fmaf(v.w, 0.f, z.w);
  }
  if (z.x != z.x) m.x = INFINITY;
  if (z.y != z.y) m.y = INFINITY;
  if (z.z != z.z) m.z = INFINITY;
  if (z.w != z.w) m.w = INFINITY;
  sm[g][4 * c4 + 0] = m.x; sm[g][4 * c4 + 1] = m.y; sm[g][4 * c4 + 2] = m.z; sm[g][4 * c4 + 3] = m.w;
  __syncthreads();
  const int d = threadIdx.x;
  partial[(int64_t)blockIdx.x * LDW_N + d] = fmaxf(fmaxf(sm[0][d], sm[1][d]), fmaxf(sm[2][d], sm[3][d]));
}

// one workgroup per column: thread i takes parts i, i + 256, .. (eight trips at 2048 parts, 288 workgroups)
__global__ __launch_bounds__(256) void ots_x_shift_kernel(const float* __restrict__ partial, int nparts, int* __restrict__ xsh) {
  __shared__ float sm[4];
  const int d = blockIdx.x;
  float m = 0.f;
  for (int b = threadIdx.x; b < nparts; b += 256) m = fmaxf(m, partial[(int64_t)b * LDW_N + d]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) xsh[d] = ls_shift(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])));
}

// ---- X: the plane images, one workgroup per piece of 32 tokens ---------------------------------------------------------
__global__ __launch_bounds__(256) void ots_split_x_kernel(const float* __restrict__ x, int64_t ldx, const int* __restrict__ xsh,
                                                           char* __restrict__ ximg) {
  char* img = ximg + (int64_t)blockIdx.x * OTS_XPIECE;
  const float* xp = x + (int64_t)blockIdx.x * LDW_KP * ldx;
  for (int i = threadIdx.x; i < LDW_N * 4; i += 256) {
    const int d = i % LDW_N, q = i / LDW_N;
    const int sh = xsh[d];
    f16x8 hv, lv;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      _Float16 h, l;
      ls_split(xp[(int64_t)(8 * q + k) * ldx + d], sh, h, l);
      hv[k] = h; lv[k] = l;
    }
    char* dst = img + ldw_x_unit(d, q);
    *reinterpret_cast<f16x8*>(dst) = hv;
    *reinterpret_cast<f16x8*>(dst + LDW_PLANE) = lv;
  }
}

// ---- the product ----------------------------------------------------------------------------------------------------
struct OtsParams {
  const float* g;
  const char* ximg;
  const int* xsh;
  float* C;                       // block b of K range `by` at C + b * blk_stride + by * slab, 288 rows of nb_cols floats
  int n_all, nb_cols, K, k_per_split;
  int64_t ldg, slab, blk_stride;
};

// 16 bytes per lane from `g` to LDS address `lds` + 16 lane (`lds` wave-uniform); opaque to the compiler on purpose, the
// waits are written out below (m0 is reserved: nothing else in this kernel reads it)
__device__ __forceinline__ void ots_dma16(const void* g, unsigned lds) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds) : "memory");
}

// the largest finite magnitude of the wave's 8 x 64 values, as fp32 bits (monotone for magnitudes), wave-uniform
__device__ __forceinline__ unsigned ots_finite_bits(float v) {
  const unsigned b = __float_as_uint(v) & 0x7fffffffu;
  return b < 0x7f800000u ? b : 0u;
}
__device__ __forceinline__ unsigned ots_wave_max_bits(const float (&v)[8]) {
  unsigned m = ots_finite_bits(v[0]);
#pragma unroll
  for (int k = 1; k < 8; ++k) m = max(m, ots_finite_bits(v[k]));
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, false));    // quad_perm [1, 0, 3, 2]
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, false));    // quad_perm [2, 3, 0, 1]
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xf, 0xf, false));   // row_half_mirror
  m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xf, 0xf, false));   // row_mirror
  const unsigned a = __builtin_amdgcn_readlane((int)m, 0), b = __builtin_amdgcn_readlane((int)m, 16);
  const unsigned c = __builtin_amdgcn_readlane((int)m, 32), d = __builtin_amdgcn_readlane((int)m, 48);
  return max(max(a, b), max(c, d));
}

// two tokens of the lane's column: their planes at 2^S as two packed halves each.  The empty asm pins the pair between
// the MFMAs where it is written (see ldx_form2).
__device__ __forceinline__ void ots_form2(float g0, float g1, int S, unsigned& hp, unsigned& lp) {
  f16x2 h, l;
  _Float16 a, b;
  ls_split_scaled(ldexpf(g0, S), a, b);
  h[0] = a; l[0] = b;
  ls_split_scaled(ldexpf(g1, S), a, b);
  h[1] = a; l[1] = b;
  hp = __builtin_bit_cast(unsigned, h);
  lp = __builtin_bit_cast(unsigned, l);
  asm volatile("" : "+v"(hp), "+v"(lp));
}

// ABLATE (timing experiments, PDN_OUTRES_TN_SPLIT_ABLATE; the results are WRONG): 1 = the planes of g are constants, g is
// never read (MFMA + LDS only); 2 = g is fetched once, before the loop (no HBM stream).
template <int ABLATE>
__global__ __launch_bounds__(512, 1) void ots_main_kernel(OtsParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[OTS_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int k_begin = by * p.k_per_split;
  const int np = ldw_range_pieces(p.K, p.k_per_split, by);      // >= 1: the host leaves no empty range
  const int c0 = bx * OTS_COLS + wave * 16;
  const bool active = c0 < p.n_all;                              // idle waves still fetch their share and meet the barriers
  const int col = c0 + r;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  const char* xsrc = p.ximg + (int64_t)(k_begin / LDW_KP) * OTS_XPIECE;
  auto dma_x = [&](int piece, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const int I = ots_x_dma_kib(e, wave);
      ots_dma16(xsrc + ots_x_dma_src(piece, I, lane), __builtin_amdgcn_readfirstlane(lds0 + ots_x_dma_lds(slot, I, 0)));
    }
  };
  const float* gsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int I = ots_g_dma_kib(i, wave);
    gsrc[i] = p.g + ots_g_src(k_begin, 0, 1, ots_g_dma_row(I, lane), p.ldg, ots_g_col(bx, ots_g_dma_chunk(I, lane), p.n_all));
  }
  auto dma_g = [&](int piece, int ring) __attribute__((always_inline)) {
    const int64_t o = (int64_t)min(piece, np - 1) * LDW_KP * p.ldg;     // (behind the last piece: a repeated fetch, never used)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      ots_dma16(gsrc[i] + o, __builtin_amdgcn_readfirstlane(lds0 + ots_g_dma_lds(ring, ots_g_dma_kib(i, wave), 0)));
  };
  const int g_lane = ots_g_read(0, wave, r, q, 0);                      // token 8 q + k: 512 k bytes further

  // ---- prologue: piece 0 of X, pieces 0 .. 3 of g, the planes of piece 0 -----------------------------------------------
  dma_x(0, 0);
  if (ABLATE != 1) { dma_g(0, 0); dma_g(1, 1); dma_g(2, 2); dma_g(3, 3); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                                      // the ring is shared: every wave's share has landed
  asm volatile("" ::: "memory");
  f16x8 bh, bl;
#pragma unroll
  for (int j = 0; j < 8; ++j) { bh[j] = (_Float16)1.f; bl[j] = (_Float16)0.5f; }
  int S = OTS_S_UNSET;
  if (ABLATE != 1) {
    float rv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) rv[k] = *reinterpret_cast<const float*>(smem + g_lane + k * 512);
    S = ots_next_scale(ots_wave_max_bits(rv), S);
    unsigned hh[4], ll[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ots_form2(rv[2 * e], rv[2 * e + 1], S, hh[e], ll[e]);
    const u32x4 hw = {hh[0], hh[1], hh[2], hh[3]}, lw = {ll[0], ll[1], ll[2], ll[3]};
    bh = __builtin_bit_cast(f16x8, hw); bl = __builtin_bit_cast(f16x8, lw);
  }

  f32x4 acc0[LDW_NT], acc1[LDW_NT];
#pragma unroll
  for (int j = 0; j < LDW_NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc0[j][i] = 0.f; acc1[j][i] = 0.f; }

  const int frag = ldw_x_frag(0, r, q);
  constexpr int TOPWAIT = ABLATE == 0 ? 2 : 0;      // memory operations a wave issues per piece behind X's

  // ---- the pieces: 18 tiles of 3 MFMAs out of slot `cur`; in their shadow X's piece s + 1 is sent to the other slot
  // (every wave is past this piece's barrier, so nobody reads that slot any more), g of piece s + 4 is sent for (into the
  // ring slot whose piece s became planes while piece s - 1 ran) and g of piece s + 1 becomes planes ----------------------
  int cur = 0;
  for (int s = 0; s < np; ++s) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TOPWAIT) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const char* fb = smem + cur + frag;
    const char* raw = smem + g_lane + ((s + 1) & (OTS_RING - 1)) * OTS_RAW;
    f16x8 xh[2], xl[2];
    u32x4 nh = __builtin_bit_cast(u32x4, bh), nl = __builtin_bit_cast(u32x4, bl);
    float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int Sn = S;
#define OTS_LOADX(X, J)                                                                                  \
  {                                                                                                      \
    xh[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024, 16));              \
    xl[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024 + LDW_PLANE, 16));  \
  }
    OTS_LOADX(0, 0)
#pragma unroll
    for (int j = 0; j < LDW_NT; ++j) {
      if (j + 1 < LDW_NT) { OTS_LOADX((j + 1) & 1, j + 1) }
      if (j == 0) {
        dma_x(min(s + 1, np - 1), 1 - (cur != 0));
        if (ABLATE == 0) dma_g(s + 4, s & (OTS_RING - 1));
        if (ABLATE != 1) {
#pragma unroll
          for (int k = 0; k < 8; ++k) rv[k] = *reinterpret_cast<const float*>(raw + k * 512);
        }
      }
      if (ABLATE != 1 && j == 2) Sn = ots_next_scale(ots_wave_max_bits(rv), S);    // the next piece's exponent
      __builtin_amdgcn_sched_barrier(0);
      acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[j & 1], bh, acc0[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[j & 1], bh, acc1[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[j & 1], bl, acc1[j], 0, 0, 0);
      if (ABLATE != 1 && (j & 3) == 0 && j >= 4) {    // a pair of tokens of the next piece, between this tile's MFMAs
        const int e = (j >> 2) - 1;                   // pair e: tokens 8 q + 2 e, + 1
        unsigned hp, lp;
        ots_form2(rv[2 * e], rv[2 * e + 1], Sn, hp, lp);
        if (e == 0) { nh.x = hp; nl.x = lp; } else if (e == 1) { nh.y = hp; nl.y = lp; }
        else if (e == 2) { nh.z = hp; nl.z = lp; } else { nh.w = hp; nl.w = lp; }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#undef OTS_LOADX
    bh = __builtin_bit_cast(f16x8, nh); bl = __builtin_bit_cast(f16x8, nl);
    if (Sn != S) {                                    // wave-uniform and rare: the sums so far move to the new scale
      if (S != OTS_S_UNSET) {
        const int dS = Sn - S;
#pragma unroll
        for (int j = 0; j < LDW_NT; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) { acc0[j][i] = ldexpf(acc0[j][i], dS); acc1[j][i] = ldexpf(acc1[j][i], dS); }
      }
      S = Sn;
    }
    cur = cur ? 0 : OTS_XPIECE;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the repeated last fetches must not outlive the workgroup's LDS

  if (!active) return;
  // ---- dW: register i of tile j = row 16 j + 4 q + i, the lane's column ------------------------------------------------
  const int Se = S == OTS_S_UNSET ? 0 : S;
  const int* __restrict__ shp = p.xsh + 4 * q;
#pragma unroll
  for (int j = 0; j < LDW_NT; ++j) {
    const int4 sv = *reinterpret_cast<const int4*>(shp + 16 * j);
    const int sh[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      p.C[ots_out_elem(by, p.slab, p.blk_stride, p.nb_cols, ldw_out_row(j, q, i), col)] =
          ldexpf(fmaf(acc1[j][i], 1.f / 2048.f, acc0[j][i]), -(Se + sh[i]));
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// PDN_OUTRES_TN_SPLIT=0: the fp32 kernel at every size (A/B switch; read once, announced)
int pdn_outres_tn_split_enabled() {
  static const int s_on = ls_env_switch("PDN_OUTRES_TN_SPLIT", 1, "the packed layer weight gradients stay on the fp32 MFMA kernel");
  return s_on;
}
// The shapes the split form takes, whatever the switch says (the workspace size must not depend on the environment): the
// packed-blocks branch of pdn_gemm_f32 (288 rows, 768 .. 8192 columns in two or more blocks) with blocks of whole waves and
// K >= 32768.  Below that the three passes over x (a launch each and 1.2 ns per token: 45 us at 32768, 25 at 16384) are no
// longer small beside what the product can save (the fp32 kernel takes 140 us for 864 columns at 32768 tokens and 70 at
// 16384, of which the split form saves somewhat over half less a fill and a drain); reasoned, not measured below 32768.
int pdn_outres_tn_split_supported(int M, int nb_cols, int nbatch, int K) {
  const int64_t n_all = (int64_t)nb_cols * nbatch;
  return (M == LDW_N && nbatch > 1 && nb_cols % 16 == 0 && n_all >= 768 && n_all <= 8192 && K >= OTS_MIN_K && K % LDW_KP == 0) ? 1 : 0;
}
int64_t pdn_outres_tn_split_extra_bytes(int K) { return ots_extra_bytes(K); }
int pdn_outres_tn_split_ranges(int n_all, int K, int plan) { return ots_ranges(n_all, plan, K / LDW_KP); }

// slabs as pdn_gemm_outres_tn_blocks_launch leaves them for `ranges` = ceil(K / k_per_split) K ranges: range s of block b at
// C + (b * ranges + s) * 288 * nb_cols.  `extra`: ots_extra_bytes(K) bytes, 16-byte aligned.
int pdn_outres_tn_split_launch(const float* X, const float* G, float* C, int n_all, int K, int64_t ldx, int64_t ldg,
                               int nb_cols, int k_per_split, void* extra, void* stream) {
  PDN_CHECK_ARG(n_all % nb_cols == 0 && pdn_outres_tn_split_supported(LDW_N, nb_cols, n_all / nb_cols, K) && k_per_split > 0 &&
                    k_per_split % LDW_KP == 0 && ((((uintptr_t)X | (uintptr_t)G | (uintptr_t)extra | (uintptr_t)C) & 15) == 0) &&
                    (ldx & 3) == 0 && (ldg & 3) == 0 && ldx >= LDW_N && ldg >= n_all,
                "pdn_outres_tn_split_launch: unsupported shape or alignment (K %d, columns %d)", K, n_all);
  static const int s_ablate = ls_env_switch("PDN_OUTRES_TN_SPLIT_ABLATE", 0,
                                            "timing ablation active, the split packed layer weight gradients are WRONG");
  hipStream_t st = (hipStream_t)stream;
  const int npieces = K / LDW_KP;
  const int ranges = (K + k_per_split - 1) / k_per_split;
  PDN_CHECK_ARG(ranges <= 65535, "pdn_outres_tn_split_launch: %d K ranges", ranges);
  char* ximg = static_cast<char*>(extra);
  int* xsh = reinterpret_cast<int*>(ximg + (int64_t)npieces * OTS_XPIECE);
  float* partial = reinterpret_cast<float*>(ximg);               // parked in the image region until the plane pass
  const int nparts = ots_partials(K);
  const int rpb = (K + nparts - 1) / nparts;
  const int nblk = (K + rpb - 1) / rpb;
  hipLaunchKernelGGL(ots_x_colmax_kernel, dim3(nblk), dim3(288), 0, st, X, ldx, K, rpb, partial);
  hipLaunchKernelGGL(ots_x_shift_kernel, dim3(LDW_N), dim3(256), 0, st, partial, nblk, xsh);
  hipLaunchKernelGGL(ots_split_x_kernel, dim3(npieces), dim3(256), 0, st, X, ldx, xsh, ximg);
  OtsParams p;
  memset(&p, 0, sizeof(p));
  p.g = G; p.ximg = ximg; p.xsh = xsh; p.C = C;
  p.n_all = n_all; p.nb_cols = nb_cols; p.K = K; p.k_per_split = k_per_split;
  p.ldg = ldg; p.slab = (int64_t)LDW_N * nb_cols; p.blk_stride = (int64_t)ranges * LDW_N * nb_cols;
  const dim3 grid((unsigned)((n_all + OTS_COLS - 1) / OTS_COLS), (unsigned)ranges), block(512);
  if (s_ablate == 1) hipLaunchKernelGGL(ots_main_kernel<1>, grid, block, 0, st, p);
  else if (s_ablate == 2) hipLaunchKernelGGL(ots_main_kernel<2>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(ots_main_kernel<0>, grid, block, 0, st, p);
  // slot 15 as well: "packed weight gradient on the output-resident TN kernel" is what bench.py asks for, whichever pipe ran it
  pdn_count(PDN_CNT_OUTRES_TN);
  pdn_count(PDN_CNT_OUTRES_TN_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
