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
//   x[:, d] 2^s(d) = xh + xl / 2048     three passes per call (csrc/split_tn_planes.hip): column maxima, exponents, 36 KiB
//                                       plane images in LDS order; ONE pass where x is an RMSNorm output given as
//                                       (rows, weight, rms): its exponents follow from the weight (stn_split_xn_kernel)
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
// Everything the loop fetches arrives by LDS-DMA (see csrc/lm_head_dw_split.hip for the order of the waits, which is written
// there once); the pieces of a tile are those of csrc/split_tn.h, every address comes from csrc/split_tn_index.h, which
// tests/outres_tn_split_check.cpp walks on the host.  Deterministic: fixed order, no atomics.
#include "split_tn.h"

struct OtsParams {
  const float* g;
  const char* ximg;
  const int* xsh;
  float* C;                       // block b of K range `by` at C + b * blk_stride + by * slab, 288 rows of nb_cols floats
  int n_all, nb_cols, K, k_per_split;
  int64_t ldg, slab, blk_stride;
};

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
// TSTORE: one block, the slabs hold the TRANSPOSE (n_all rows of 288 floats; a lane's four registers of a tile are sixteen
// consecutive bytes of its column's row): dW_down^T = g2^T h, whose slabs are then dW_down's, row-major.
template <int ABLATE, bool TSTORE = false>
__global__ __launch_bounds__(512, 1) void ots_main_kernel(OtsParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[stn_lds(OTS_XKIB)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int k_begin = by * p.k_per_split;
  const int np = stn_range_pieces(p.K, p.k_per_split, by);      // >= 1: the host leaves no empty range
  const int c0 = bx * STN_COLS + wave * 16;
  const bool active = c0 < p.n_all;                              // idle waves still fetch their share and meet the barriers
  const int col = c0 + r;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  const char* xsrc = p.ximg + (int64_t)(k_begin / STN_KP) * stn_xpiece(OTS_XKIB);
  auto dma_x = [&](int piece, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const int I = stn_x_dma_kib(e, wave, OTS_XKIB);
      split_dma16(xsrc + stn_x_dma_src(piece, I, lane, OTS_XKIB), __builtin_amdgcn_readfirstlane(lds0 + stn_x_dma_lds(slot, I, 0, OTS_XKIB)));
    }
  };
  const float* gsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int I = stn_raw_dma_kib(i, wave);
    gsrc[i] = p.g + stn_raw_src(k_begin, 0, 1, stn_raw_dma_row(I, lane), p.ldg, stn_raw_col(bx, stn_raw_dma_chunk(I, lane), p.n_all));
  }
  auto dma_g = [&](int piece, int ring) __attribute__((always_inline)) {
    const int64_t o = (int64_t)min(piece, np - 1) * STN_KP * p.ldg;     // (behind the last piece: a repeated fetch, never used)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      split_dma16(gsrc[i] + o, __builtin_amdgcn_readfirstlane(lds0 + stn_raw_dma_lds(ring, stn_raw_dma_kib(i, wave), 0, OTS_XKIB)));
  };
  const int g_lane = stn_raw_read(0, wave, r, q, 0, OTS_XKIB);                      // token 8 q + k: 512 k bytes further

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
    bh = stn_pack4(hh[0], hh[1], hh[2], hh[3]); bl = stn_pack4(ll[0], ll[1], ll[2], ll[3]);
  }

  f32x4 acc0[STN_NT], acc1[STN_NT];
  STN_CLEAR(acc0, acc1)

  const int frag = stn_x_frag(0, r, q);
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
    const char* raw = smem + g_lane + ((s + 1) & (STN_RING - 1)) * STN_RAW;
    f16x8 xh[2], xl[2];
    u32x4 nh = __builtin_bit_cast(u32x4, bh), nl = __builtin_bit_cast(u32x4, bl);
    float rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int Sn = S;
    stn_load_frag(fb, 0, xh[0], xl[0]);
#pragma unroll
    for (int j = 0; j < STN_NT; ++j) {
      if (j + 1 < STN_NT) stn_load_frag(fb, j + 1, xh[(j + 1) & 1], xl[(j + 1) & 1]);
      if (j == 0) {
        dma_x(min(s + 1, np - 1), 1 - (cur != 0));
        if (ABLATE == 0) dma_g(s + 4, s & (STN_RING - 1));
        if (ABLATE != 1) {
#pragma unroll
          for (int k = 0; k < 8; ++k) rv[k] = *reinterpret_cast<const float*>(raw + k * 512);
        }
      }
      if (ABLATE != 1 && j == 2) Sn = ots_next_scale(ots_wave_max_bits(rv), S);    // the next piece's exponent
      __builtin_amdgcn_sched_barrier(0);
      stn_mfma3(xh[j & 1], xl[j & 1], bh, bl, acc0[j], acc1[j]);
      if (ABLATE != 1 && (j & 3) == 0 && j >= 4) {    // a pair of tokens of the next piece, between this tile's MFMAs
        const int e = (j >> 2) - 1;                   // pair e: tokens 8 q + 2 e, + 1
        unsigned hp, lp;
        ots_form2(rv[2 * e], rv[2 * e + 1], Sn, hp, lp);
        if (e == 0) { nh.x = hp; nl.x = lp; } else if (e == 1) { nh.y = hp; nl.y = lp; }
        else if (e == 2) { nh.z = hp; nl.z = lp; } else { nh.w = hp; nl.w = lp; }
        stn_sched_pair();
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    bh = __builtin_bit_cast(f16x8, nh); bl = __builtin_bit_cast(f16x8, nl);
    if (Sn != S) {                                    // wave-uniform and rare: the sums so far move to the new scale
      if (S != OTS_S_UNSET) {
        const int dS = Sn - S;
#pragma unroll
        for (int j = 0; j < STN_NT; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) { acc0[j][i] = ldexpf(acc0[j][i], dS); acc1[j][i] = ldexpf(acc1[j][i], dS); }
      }
      S = Sn;
    }
    cur = cur ? 0 : stn_xpiece(OTS_XKIB);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the repeated last fetches must not outlive the workgroup's LDS

  if (!active) return;
  // ---- dW: register i of tile j = row 16 j + 4 q + i, the lane's column ------------------------------------------------
  const int Se = S == OTS_S_UNSET ? 0 : S;
  const int* __restrict__ shp = p.xsh + 4 * q;
#pragma unroll
  for (int j = 0; j < STN_NT; ++j) {
    const int4 sv = *reinterpret_cast<const int4*>(shp + 16 * j);
    const int sh[4] = {sv.x, sv.y, sv.z, sv.w};
    if (TSTORE) {
      float4 o;
      o.x = stn_unscale(acc1[j][0], acc0[j][0], Se + sh[0]); o.y = stn_unscale(acc1[j][1], acc0[j][1], Se + sh[1]);
      o.z = stn_unscale(acc1[j][2], acc0[j][2], Se + sh[2]); o.w = stn_unscale(acc1[j][3], acc0[j][3], Se + sh[3]);
      *reinterpret_cast<float4*>(p.C + ots_out_elem_t(by, p.slab, stn_out_row(j, q, 0), col)) = o;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        p.C[ots_out_elem(by, p.slab, p.blk_stride, p.nb_cols, stn_out_row(j, q, i), col)] =
            stn_unscale(acc1[j][i], acc0[j][i], Se + sh[i]);
    }
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
  return (M == STN_N && nbatch > 1 && nb_cols % 16 == 0 && n_all >= 768 && n_all <= 8192 && K >= OTS_MIN_K && K % STN_KP == 0) ? 1 : 0;
}
int64_t pdn_outres_tn_split_extra_bytes(int K) { return stn_extra_bytes(K, OTS_XKIB); }
int pdn_outres_tn_split_ranges(int n_all, int K, int plan) { return ots_ranges(n_all, plan, K / STN_KP); }

// slabs as pdn_gemm_outres_tn_blocks_launch leaves them for `ranges` = ceil(K / k_per_split) K ranges: range s of block b at
// C + (b * ranges + s) * 288 * nb_cols.  `extra`: stn_extra_bytes(K, OTS_XKIB) bytes, 16-byte aligned.
// (norm_w, rms) given: X holds the rows BEFORE an RMSNorm whose output is the operand (one plane launch instead of three)
static int ots_launch(const float* X, const float* norm_w, const float* rms, const float* G, float* C, int n_all, int K,
                      int64_t ldx, int64_t ldg, int nb_cols, int k_per_split, void* extra, void* stream) {
  PDN_CHECK_ARG(n_all % nb_cols == 0 && pdn_outres_tn_split_supported(STN_N, nb_cols, n_all / nb_cols, K) && k_per_split > 0 &&
                    k_per_split % STN_KP == 0 && ((((uintptr_t)X | (uintptr_t)G | (uintptr_t)extra | (uintptr_t)C) & 15) == 0) &&
                    (ldx & 3) == 0 && (ldg & 3) == 0 && ldx >= STN_N && ldg >= n_all,
                "pdn_outres_tn_split_launch: unsupported shape or alignment (K %d, columns %d)", K, n_all);
  static const int s_ablate = ls_env_switch("PDN_OUTRES_TN_SPLIT_ABLATE", 0,
                                            "timing ablation active, the split packed layer weight gradients are WRONG");
  const int ranges = (K + k_per_split - 1) / k_per_split;
  PDN_CHECK_ARG(ranges <= 65535, "pdn_outres_tn_split_launch: %d K ranges", ranges);
  OtsParams p;
  memset(&p, 0, sizeof(p));
  p.g = G; p.ximg = static_cast<const char*>(extra);
  p.xsh = norm_w ? stn_xn_planes_launch(X, ldx, norm_w, rms, K, extra, stream) : stn_x_planes_launch(X, ldx, K, extra, nullptr, nullptr, stream);
  p.C = C;
  p.n_all = n_all; p.nb_cols = nb_cols; p.K = K; p.k_per_split = k_per_split;
  p.ldg = ldg; p.slab = (int64_t)STN_N * nb_cols; p.blk_stride = (int64_t)ranges * STN_N * nb_cols;
  STN_LAUNCH_ABLATE(ots_main_kernel, s_ablate, dim3((unsigned)((n_all + STN_COLS - 1) / STN_COLS), (unsigned)ranges), stream, p);
  // slot 15 as well: "packed weight gradient on the output-resident TN kernel" is what bench.py asks for, whichever pipe ran it
  pdn_count(PDN_CNT_OUTRES_TN);
  pdn_count(PDN_CNT_OUTRES_TN_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
int pdn_outres_tn_split_launch(const float* X, const float* G, float* C, int n_all, int K, int64_t ldx, int64_t ldg,
                               int nb_cols, int k_per_split, void* extra, void* stream) {
  return ots_launch(X, nullptr, nullptr, G, C, n_all, K, ldx, ldg, nb_cols, k_per_split, extra, stream);
}
int pdn_outres_tn_split_norm_launch(const float* x, const float* norm_w, const float* rms, const float* G, float* C, int n_all,
                                    int K, int64_t ldx, int64_t ldg, int nb_cols, int k_per_split, void* extra, void* stream) {
  PDN_CHECK_ARG(norm_w && rms && (((uintptr_t)norm_w | (uintptr_t)rms) & 3) == 0, "pdn_outres_tn_split_norm_launch: norm operands");
  return ots_launch(x, norm_w, rms, G, C, n_all, K, ldx, ldg, nb_cols, k_per_split, extra, stream);
}

// ---- the down-projection weight gradient: dW_down (M x 288) = h^T g2 as (g2^T h)^T, one block, transposed store ----------
// g2 (K x 288) is the plane-image operand with one exponent per column, h (K x M) the raw one under the per-wave running
// exponent.  M in whole waves from 512 to 1024 columns (four to eight column workgroups: 32 .. 64 K ranges in one round;
// narrower outputs have too few columns to pay for the passes, wider ones would get fewer, longer ranges than any measured).
int pdn_down_dw_split_supported(int M, int N, int K) {
  return (N == STN_N && M % 16 == 0 && M >= 512 && M <= 1024 && K >= OTS_MIN_K && K % STN_KP == 0) ? 1 : 0;
}
int pdn_down_dw_split_ranges(int M, int K) { return ots_t_ranges(M, K / STN_KP); }

// slabs: K range s at C + s * M * 288, M rows of 288 floats.  `extra`: stn_extra_bytes(K, OTS_XKIB) bytes, 16-byte aligned.
int pdn_down_dw_split_launch(const float* G2, const float* H, float* C, int M, int K, int64_t ldx, int64_t ldg, int k_per_split,
                             void* extra, void* stream) {
  PDN_CHECK_ARG(pdn_down_dw_split_supported(M, STN_N, K) && k_per_split > 0 && k_per_split % STN_KP == 0 &&
                    ((((uintptr_t)G2 | (uintptr_t)H | (uintptr_t)extra | (uintptr_t)C) & 15) == 0) && (ldx & 3) == 0 &&
                    (ldg & 3) == 0 && ldx >= STN_N && ldg >= M,
                "pdn_down_dw_split_launch: unsupported shape or alignment (K %d, rows %d)", K, M);
  const int ranges = (K + k_per_split - 1) / k_per_split;
  PDN_CHECK_ARG(ranges <= OTS_MAX_RANGES, "pdn_down_dw_split_launch: %d K ranges", ranges);
  OtsParams p;
  memset(&p, 0, sizeof(p));
  p.g = H; p.ximg = static_cast<const char*>(extra); p.xsh = stn_x_planes_launch(G2, ldx, K, extra, nullptr, nullptr, stream);
  p.C = C;
  p.n_all = M; p.nb_cols = M; p.K = K; p.k_per_split = k_per_split;
  p.ldg = ldg; p.slab = (int64_t)STN_N * M; p.blk_stride = 0;
  hipLaunchKernelGGL((ots_main_kernel<0, true>), dim3((unsigned)((M + STN_COLS - 1) / STN_COLS), (unsigned)ranges), dim3(512), 0,
                     (hipStream_t)stream, p);
  pdn_count(PDN_CNT_DOWN_DW_SPLIT);                 // here only: slots 15 and 42 stay the packed products'
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
