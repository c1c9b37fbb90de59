// lm_head weight gradient on split-fp16 MFMA at fp32 accuracy (gfx950 only):
//
//   dW[d][v] = sc * sum_t x[t][d] g[t][v],   g = exp(logit[t][v] - lse[t]) - [v == target[t]],   sc = gscale * upstream
//   colsum[v] = sc * sum_t g[t][v]
//
// the product of gemm_outres_tn_kernel<.., CE> (csrc/gemm_outres.hip; `A^T @ grad` of pydynet/core/tensor.py:672-675 behind
// the cross entropy of nn/functional.py:364-381), routed here by pdn_linear_ce_backward_f32 (csrc/gemm.hip) for the
// many-row shapes of a training step.  Both operands are fp16 planes, like the forward and the input gradient
// (csrc/lm_head_split.hip, csrc/lm_head_dx_split.hip):
//
//   g 2^15 = gh + gl / 2048                       formed ON THE FLY from the fp32 logits (one fma, one exp2, one
//                                                 select-subtract: ce_unscaled of the fp32 kernel), |g| <= 1
//   x[:, d] 2^s(d) = xh + xl / 2048               two passes per call: column maxima, then the planes; one power of two
//                                                 per COLUMN d of x = per row of dW
//   dW 2^(15 + s(d)) / sc = xh gh + (xh gl + xl gh) / 2048
//
// Structure: output-resident.  A wave owns SIXTEEN vocabulary columns and all 288 rows of dW of them on
// `v_mfma_f32_16x16x32_f16`: 18 tiles x 4 registers x 2 sums = 144 accumulators, eight waves = 128 columns per workgroup,
// K = tokens cut into the ranges of pdn_gemm_outres_tn_plan over grid.y (the slabs and column-sum slabs of the fp32 kernel,
// combined by the same gemm_splitk_reduce_kernel launches).  x^T's tile is the MFMA A operand, g the B operand: a lane
// owns ONE column v = lane & 15 and four consecutive rows per tile.
// Everything the loop fetches arrives by LDS-DMA (`global_load_lds_dwordx4` from inline assembly, see
// csrc/lm_head_dx_split.hip for why not the builtin), all of it shared by the workgroup:
//   * X's planes as 37 KiB images in LDS order (written by the plane pass), two slots; the image's tail carries -lse log2 e
//     and the targets of the NEXT piece's 32 tokens;
//   * the logits, read exactly once in whole 512-byte row segments, into a ring of four 16 KiB pieces; the 16-byte chunks
//     of a row are XOR-swizzled on the source side (csrc/lm_head_dw_split_index.h) so that the transposed ds_read_b32 by
//     which lane (v, q) fetches the logits of tokens 8 q .. 8 q + 7 is conflict free.
// Per piece a wave issues X's piece s + 1 (five instructions) and THEN its share of the logits of piece s + 4 (two); loads
// retire in order, so the one `s_waitcnt vmcnt(2)` in front of the piece's barrier means "my share of X's piece s has
// landed" and, with it, everything older: the logits of piece s + 2 and before; the barrier extends that to every wave's
// share.  The ring slot of piece s was turned into planes while piece s - 1 ran, so after the barrier of piece s it is free
// for piece s + 4.  Deterministic: fixed order, no atomics.
#include "common.h"
#include "lm_head_split.h"
#include "lm_head_dw_split_index.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

#define LDW_ES 15                         // g is scaled by 2^15
#define LDW_L2E 1.4426950408889634f

// ---- X: column maxima over a range of rows (partial), then the exponent of every column -----------------------------
// 288 threads: thread (c4 = tid % 72, g = tid / 72) takes the float4 c4 of rows g, g + 4, .. of the block's range
__global__ __launch_bounds__(288) void ldw_x_colmax_kernel(const float* __restrict__ x, int64_t ldx, int rows, int rows_per_block,
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

// one workgroup per column: thread i takes parts i, i + 256, .. (eight trips at 2048 parts over 288 workgroups; nine
// workgroups of 32 columns x 8 part groups made 256 dependent trips, 51 us of latency)
__global__ __launch_bounds__(256) void ldw_x_shift_kernel(const float* __restrict__ partial, int nparts, int* __restrict__ xsh) {
  __shared__ float sm[4];
  const int d = blockIdx.x;
  float m = 0.f;
  for (int b = threadIdx.x; b < nparts; b += 256) m = fmaxf(m, partial[(int64_t)b * LDW_N + d]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) xsh[d] = ls_shift(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])));
}

// ---- X: the plane images, one workgroup per piece of 32 tokens; the tail holds the row statistics of the NEXT piece ------
__global__ __launch_bounds__(256) void ldw_split_x_kernel(const float* __restrict__ x, int64_t ldx, const int* __restrict__ xsh,
                                                           const float* __restrict__ lse, const int64_t* __restrict__ targets,
                                                           int rows, char* __restrict__ ximg) {
  char* img = ximg + (int64_t)blockIdx.x * LDW_XPIECE;
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
  // tail: 1 KiB = 256 dwords; dwords 0..31 -lse log2 e, 32..63 the targets, the rest zero
  {
    const int i = threadIdx.x;
    const int64_t t = ((int64_t)blockIdx.x + 1) * LDW_KP + (i & 31);
    unsigned v = 0u;
    if (i < 64 && t < rows) v = i < 32 ? __float_as_uint(-LDW_L2E * lse[t]) : (unsigned)(int)targets[t];
    reinterpret_cast<unsigned*>(img + LDW_TAIL)[i] = v;
  }
}

// ---- the product ----------------------------------------------------------------------------------------------------
struct LdwParams {
  const float* logits;
  const char* ximg;
  const int* xsh;
  const float* lse;
  const int64_t* targets;
  const float* gdev;
  float* C;                       // slab of K range `by` at C + by * slab, 288 rows of V floats
  float* colsum;                  // [ranges][V] or null
  int V, K, k_per_split;
  int64_t ldl, slab;
  float gscale;
};

// 16 bytes per lane from `g` to LDS address `lds` + 16 lane (`lds` wave-uniform); opaque to the compiler on purpose, the
// waits are written out below (m0 is reserved: nothing else in this kernel reads it)
__device__ __forceinline__ void ldw_dma16(const void* g, unsigned lds) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds) : "memory");
}

// two tokens of the lane's column: g as the fp32 kernel forms it, their sum for the column sum, their planes at 2^15 as two
// packed halves each.  The empty asm pins the pair between the MFMAs where it is written (see ldx_form2).
__device__ __forceinline__ void ldw_form2(float x0, float x1, float n0, float n1, bool t0, bool t1, float& gsum, unsigned& hp,
                                          unsigned& lp) {
  const float e0 = __builtin_amdgcn_exp2f(fmaf(x0, LDW_L2E, n0));
  const float e1 = __builtin_amdgcn_exp2f(fmaf(x1, LDW_L2E, n1));
  const float g0 = t0 ? e0 - 1.f : e0;
  const float g1 = t1 ? e1 - 1.f : e1;
  gsum = g0 + g1;
  f16x2 h, l;
  _Float16 a, b;
  ls_split_scaled(g0 * (float)(1 << LDW_ES), a, b);
  h[0] = a; l[0] = b;
  ls_split_scaled(g1 * (float)(1 << LDW_ES), a, b);
  h[1] = a; l[1] = b;
  hp = __builtin_bit_cast(unsigned, h);
  lp = __builtin_bit_cast(unsigned, l);
  asm volatile("" : "+v"(hp), "+v"(lp));
}

// ABLATE (timing experiments, PDN_LMHEAD_DW_SPLIT_ABLATE; the results are WRONG): 1 = the planes of g are constants, the
// logits are never read (MFMA + LDS only); 2 = the logits are fetched once, before the loop (no HBM stream).
template <int ABLATE>
__global__ __launch_bounds__(512, 1) void ldw_main_kernel(LdwParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[LDW_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int k_begin = by * p.k_per_split;
  const int np = ldw_range_pieces(p.K, p.k_per_split, by);      // >= 1: the plan leaves no empty range
  const int c0 = bx * LDW_COLS + wave * 16;
  const bool active = c0 < p.V;                                   // idle waves still fetch their share and meet the barriers
  const int col = c0 + r;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  const float ce_sc = p.gscale * (p.gdev ? p.gdev[0] : 1.f);

  // the row statistics of the range's first piece come straight from memory (later ones ride in the images' tails)
  float n8[8];
  int t8[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    n8[k] = -LDW_L2E * p.lse[k_begin + 8 * q + k];
    t8[k] = (int)p.targets[k_begin + 8 * q + k];
  }

  const char* xsrc = p.ximg + (int64_t)(k_begin / LDW_KP) * LDW_XPIECE;
  auto dma_x = [&](int piece, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const int I = ldw_x_dma_kib(e, wave);
      ldw_dma16(xsrc + ldw_x_dma_src(piece, I, lane), __builtin_amdgcn_readfirstlane(lds0 + ldw_x_dma_lds(slot, I, 0)));
    }
  };
  const float* lsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int I = ldw_raw_dma_kib(i, wave);
    lsrc[i] = p.logits + (int64_t)ldw_raw_row(k_begin, 0, 1, ldw_raw_dma_row(I, lane)) * p.ldl +
              ldw_raw_col(bx, ldw_raw_dma_chunk(I, lane), p.V);
  }
  auto dma_raw = [&](int piece, int ring) __attribute__((always_inline)) {
    const int64_t o = (int64_t)min(piece, np - 1) * LDW_KP * p.ldl;     // (behind the last piece: a repeated fetch, never used)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      ldw_dma16(lsrc[i] + o, __builtin_amdgcn_readfirstlane(lds0 + ldw_raw_dma_lds(ring, ldw_raw_dma_kib(i, wave), 0)));
  };
  const int raw_lane = ldw_raw_read(0, wave, r, q, 0);               // token 8 q + k: 512 k bytes further

  // ---- prologue: piece 0 of X, pieces 0 .. 3 of the logits, the planes of piece 0 ------------------------------------
  dma_x(0, 0);
  if (ABLATE != 1) { dma_raw(0, 0); dma_raw(1, 1); dma_raw(2, 2); dma_raw(3, 3); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                                      // the ring is shared: every wave's share has landed
  asm volatile("" ::: "memory");
  f16x8 bh, bl;
#pragma unroll
  for (int j = 0; j < 8; ++j) { bh[j] = (_Float16)1.f; bl[j] = (_Float16)0.5f; }
  float csum = 0.f;
  if (ABLATE != 1) {
    unsigned hh[4], ll[4];
    float ps[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x0 = *reinterpret_cast<const float*>(smem + raw_lane + (2 * e) * 512);
      const float x1 = *reinterpret_cast<const float*>(smem + raw_lane + (2 * e + 1) * 512);
      ldw_form2(x0, x1, n8[2 * e], n8[2 * e + 1], t8[2 * e] == col, t8[2 * e + 1] == col, ps[e], hh[e], ll[e]);
    }
    csum = (ps[0] + ps[1]) + (ps[2] + ps[3]);
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
  // (every wave is past this piece's barrier, so nobody reads that slot any more), the logits of piece s + 4 are sent for
  // (into the ring slot whose piece s became planes while piece s - 1 ran) and those of piece s + 1 become planes ---------
  int cur = 0;
  for (int s = 0; s < np; ++s) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TOPWAIT) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const char* fb = smem + cur + frag;
    const char* tail = smem + cur + LDW_TAIL + 32 * q;               // the next piece's tokens 8 q .. 8 q + 7
    const char* raw = smem + raw_lane + ((s + 1) & (LDW_RING - 1)) * LDW_RAW;
    const bool live = s + 1 < np;                                    // (behind the last piece: planes nobody multiplies)
    f16x8 xh[2], xl[2];
    u32x4 nh = __builtin_bit_cast(u32x4, bh), nl = __builtin_bit_cast(u32x4, bl);
    float rx0 = 0.f, rx1 = 0.f;
    float2 rn = make_float2(0.f, 0.f);
    int2 rt = make_int2(0, 0);
    float zp = 0.f, zq = 0.f;
#define LDW_LOADX(X, J)                                                                                  \
  {                                                                                                      \
    xh[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024, 16));              \
    xl[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024 + LDW_PLANE, 16));  \
  }
    LDW_LOADX(0, 0)
#pragma unroll
    for (int j = 0; j < LDW_NT; ++j) {
      if (j + 1 < LDW_NT) { LDW_LOADX((j + 1) & 1, j + 1) }
      if (j == 0) {
        dma_x(min(s + 1, np - 1), 1 - (cur != 0));
        if (ABLATE == 0) dma_raw(s + 4, s & (LDW_RING - 1));
      }
      if (ABLATE != 1 && (j & 3) == 0 && j < 16) {    // what the pair formed two tiles on needs
        const int e = j >> 2;
        rx0 = *reinterpret_cast<const float*>(raw + (2 * e) * 512);
        rx1 = *reinterpret_cast<const float*>(raw + (2 * e + 1) * 512);
        rn = *reinterpret_cast<const float2*>(__builtin_assume_aligned(tail + 8 * e, 8));
        rt = *reinterpret_cast<const int2*>(__builtin_assume_aligned(tail + 128 + 8 * e, 8));
      }
      __builtin_amdgcn_sched_barrier(0);
      acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[j & 1], bh, acc0[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[j & 1], bh, acc1[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[j & 1], bl, acc1[j], 0, 0, 0);
      if (ABLATE != 1 && (j & 3) == 2 && j < 16) {    // a pair of tokens of the next piece, between this tile's MFMAs
        const int e = j >> 2;                         // pair e: tokens 8 q + 2 e, + 1
        unsigned hp, lp;
        float ps;
        ldw_form2(rx0, rx1, rn.x, rn.y, rt.x == col, rt.y == col, ps, hp, lp);
        if (e == 0) { nh.x = hp; nl.x = lp; zp = ps; } else if (e == 1) { nh.y = hp; nl.y = lp; zp += ps; }
        else if (e == 2) { nh.z = hp; nl.z = lp; zq = ps; } else { nh.w = hp; nl.w = lp; csum += live ? zp + (zq + ps) : 0.f; }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#undef LDW_LOADX
    bh = __builtin_bit_cast(f16x8, nh); bl = __builtin_bit_cast(f16x8, nl);
    cur = cur ? 0 : LDW_XPIECE;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the repeated last fetches must not outlive the workgroup's LDS

  if (!active) return;
  // ---- column sums: the four lane quarters saw disjoint tokens ------------------------------------------------------
  if (p.colsum) {
    float cs = csum + __shfl_xor(csum, 16, 64);
    cs += __shfl_xor(cs, 32, 64);
    if (q == 0) p.colsum[(int64_t)by * p.V + col] = cs * ce_sc;
  }
  // ---- dW: register i of tile j = row 16 j + 4 q + i, the lane's column ------------------------------------------------
  const int* __restrict__ shp = p.xsh + 4 * q;
#pragma unroll
  for (int j = 0; j < LDW_NT; ++j) {
    const int4 sv = *reinterpret_cast<const int4*>(shp + 16 * j);
    const int sh[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      p.C[ldw_out_elem(by, p.slab, ldw_out_row(j, q, i), p.V, col)] =
          ldexpf(fmaf(acc1[j][i], 1.f / 2048.f, acc0[j][i]), -(LDW_ES + sh[i])) * ce_sc;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
// PDN_LMHEAD_DW_SPLIT=0: the fp32 kernel at every size (A/B switch; read once, announced)
int pdn_outres_ce_dw_split_enabled() {
  static const int s_on = ls_env_switch("PDN_LMHEAD_DW_SPLIT", 1, "the lm_head weight gradient stays on the fp32 MFMA kernel");
  return s_on;
}
// The shapes the split form takes, whatever the switch says (the workspace size must not depend on the environment).
// rows >= 32768: below, a K range is a few hundred pieces at most and the two passes over x are no longer small beside
// the product (reasoned from the passes' 0.15 ms, not measured below that size); V >= 128: one whole column block.
int pdn_outres_ce_dw_split_supported(int64_t rows, int V, int in_features) {
  return (in_features == LDW_N && V >= LDW_MIN_V && V % 32 == 0 && rows >= LDW_MIN_ROWS && rows % LDW_KP == 0 &&
          rows < (1ll << 31) && (int64_t)LDW_N * V < (1ll << 30)) ? 1 : 0;
}
int64_t pdn_outres_ce_dw_split_extra_bytes(int64_t rows) { return ldw_extra_bytes(rows); }

// slabs / colsum as pdn_outres_ce_dw_launch leaves them: range s (k_per_split tokens) at C + s * slab, colsum [ranges][V].
// `extra`: ldw_extra_bytes(rows) bytes, 16-byte aligned.
int pdn_outres_ce_dw_split_launch(const float* x, int64_t ldx, const float* logits, float* C, int V, int64_t rows,
                                  int64_t slab, int k_per_split, const float* lse, const int64_t* targets, float gscale,
                                  const float* gdev, float* colsum, void* extra, void* stream) {
  PDN_CHECK_ARG(pdn_outres_ce_dw_split_supported(rows, V, LDW_N) && k_per_split > 0 && k_per_split % LDW_KP == 0 &&
                    ((((uintptr_t)x | (uintptr_t)logits | (uintptr_t)extra) & 15) == 0) && (ldx & 3) == 0,
                "pdn_outres_ce_dw_split_launch: unsupported shape or alignment (rows %lld, V %d)", (long long)rows, V);
  static const int s_ablate = ls_env_switch("PDN_LMHEAD_DW_SPLIT_ABLATE", 0,
                                            "timing ablation active, dW and dbias of the split lm_head weight gradient are WRONG");
  hipStream_t st = (hipStream_t)stream;
  const int M = (int)rows, npieces = M / LDW_KP;
  char* ximg = static_cast<char*>(extra);
  int* xsh = reinterpret_cast<int*>(ximg + (int64_t)npieces * LDW_XPIECE);
  float* partial = reinterpret_cast<float*>(ximg);               // parked in the image region until the plane pass
  const int nparts = ldw_partials(rows);
  const int rpb = (M + nparts - 1) / nparts;
  hipLaunchKernelGGL(ldw_x_colmax_kernel, dim3((M + rpb - 1) / rpb), dim3(288), 0, st, x, ldx, M, rpb, partial);
  hipLaunchKernelGGL(ldw_x_shift_kernel, dim3(LDW_N), dim3(256), 0, st, partial, (M + rpb - 1) / rpb, xsh);
  hipLaunchKernelGGL(ldw_split_x_kernel, dim3(npieces), dim3(256), 0, st, x, ldx, xsh, lse, targets, M, ximg);
  LdwParams p;
  memset(&p, 0, sizeof(p));
  p.logits = logits; p.ximg = ximg; p.xsh = xsh; p.lse = lse; p.targets = targets; p.gdev = gdev; p.C = C; p.colsum = colsum;
  p.V = V; p.K = M; p.k_per_split = k_per_split; p.ldl = V; p.slab = slab; p.gscale = gscale;
  const dim3 grid((unsigned)((V + LDW_COLS - 1) / LDW_COLS), (unsigned)((M + k_per_split - 1) / k_per_split)), block(512);
  if (s_ablate == 1) hipLaunchKernelGGL(ldw_main_kernel<1>, grid, block, 0, st, p);
  else if (s_ablate == 2) hipLaunchKernelGGL(ldw_main_kernel<2>, grid, block, 0, st, p);
  else hipLaunchKernelGGL(ldw_main_kernel<0>, grid, block, 0, st, p);
  // slot 13 as well: "lm_head weight gradient with the CE gradient inside" is what bench.py asks for, whichever pipe ran it
  pdn_count(PDN_CNT_CE_DW);
  pdn_count(PDN_CNT_CE_DW_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
