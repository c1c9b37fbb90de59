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
//   * X's planes as 37 KiB images in LDS order (written by the plane pass of csrc/split_tn_planes.hip), two slots; the
//     image's tail carries -lse log2 e and the targets of the NEXT piece's 32 tokens;
//   * the logits, read exactly once in whole 512-byte row segments, into a ring of four 16 KiB pieces; the 16-byte chunks
//     of a row are XOR-swizzled on the source side (csrc/split_tn_index.h) so that the transposed ds_read_b32 by
//     which lane (v, q) fetches the logits of tokens 8 q .. 8 q + 7 is conflict free.
// Per piece a wave issues X's piece s + 1 (five instructions) and THEN its share of the logits of piece s + 4 (two); loads
// retire in order, so the one `s_waitcnt vmcnt(2)` in front of the piece's barrier means "my share of X's piece s has
// landed" and, with it, everything older: the logits of piece s + 2 and before; the barrier extends that to every wave's
// share.  The ring slot of piece s was turned into planes while piece s - 1 ran, so after the barrier of piece s it is free
// for piece s + 4.  Deterministic: fixed order, no atomics.
// The packed layer weight gradients (csrc/outres_tn_split.hip) run the same pipeline on raw g; the two main kernels stay
// apart (through one shared loop template they compiled to other schedules than these), what they share is in
// csrc/split_tn.h (LDS-DMA, fragment loads, the tile, the scheduling pattern), csrc/split_tn_planes.hip (the passes over x)
// and csrc/split_tn_index.h (every address, walked on the host by tests/lm_head_dw_split_check.cpp).
#include "split_tn.h"

#define LDW_ES 15                         // g is scaled by 2^15
#define LDW_L2E 1.4426950408889634f

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
  __shared__ __attribute__((aligned(1024))) char smem[stn_lds(LDW_XKIB)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int k_begin = by * p.k_per_split;
  const int np = stn_range_pieces(p.K, p.k_per_split, by);      // >= 1: the plan leaves no empty range
  const int c0 = bx * STN_COLS + wave * 16;
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

  const char* xsrc = p.ximg + (int64_t)(k_begin / STN_KP) * stn_xpiece(LDW_XKIB);
  auto dma_x = [&](int piece, int slot) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const int I = stn_x_dma_kib(e, wave, LDW_XKIB);
      split_dma16(xsrc + stn_x_dma_src(piece, I, lane, LDW_XKIB), __builtin_amdgcn_readfirstlane(lds0 + stn_x_dma_lds(slot, I, 0, LDW_XKIB)));
    }
  };
  const float* lsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int I = stn_raw_dma_kib(i, wave);
    lsrc[i] = p.logits + (int64_t)stn_raw_row(k_begin, 0, 1, stn_raw_dma_row(I, lane)) * p.ldl +
              stn_raw_col(bx, stn_raw_dma_chunk(I, lane), p.V);
  }
  auto dma_raw = [&](int piece, int ring) __attribute__((always_inline)) {
    const int64_t o = (int64_t)min(piece, np - 1) * STN_KP * p.ldl;     // (behind the last piece: a repeated fetch, never used)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      split_dma16(lsrc[i] + o, __builtin_amdgcn_readfirstlane(lds0 + stn_raw_dma_lds(ring, stn_raw_dma_kib(i, wave), 0, LDW_XKIB)));
  };
  const int raw_lane = stn_raw_read(0, wave, r, q, 0, LDW_XKIB);               // token 8 q + k: 512 k bytes further

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
    bh = stn_pack4(hh[0], hh[1], hh[2], hh[3]); bl = stn_pack4(ll[0], ll[1], ll[2], ll[3]);
  }

  f32x4 acc0[STN_NT], acc1[STN_NT];
  STN_CLEAR(acc0, acc1)

  const int frag = stn_x_frag(0, r, q);
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
    const char* raw = smem + raw_lane + ((s + 1) & (STN_RING - 1)) * STN_RAW;
    const bool live = s + 1 < np;                                    // (behind the last piece: planes nobody multiplies)
    f16x8 xh[2], xl[2];
    u32x4 nh = __builtin_bit_cast(u32x4, bh), nl = __builtin_bit_cast(u32x4, bl);
    float rx0 = 0.f, rx1 = 0.f;
    float2 rn = make_float2(0.f, 0.f);
    int2 rt = make_int2(0, 0);
    float zp = 0.f, zq = 0.f;
    stn_load_frag(fb, 0, xh[0], xl[0]);
#pragma unroll
    for (int j = 0; j < STN_NT; ++j) {
      if (j + 1 < STN_NT) stn_load_frag(fb, j + 1, xh[(j + 1) & 1], xl[(j + 1) & 1]);
      if (j == 0) {
        dma_x(min(s + 1, np - 1), 1 - (cur != 0));
        if (ABLATE == 0) dma_raw(s + 4, s & (STN_RING - 1));
      }
      if (ABLATE != 1 && (j & 3) == 0 && j < 16) {    // what the pair formed two tiles on needs
        const int e = j >> 2;
        rx0 = *reinterpret_cast<const float*>(raw + (2 * e) * 512);
        rx1 = *reinterpret_cast<const float*>(raw + (2 * e + 1) * 512);
        rn = *reinterpret_cast<const float2*>(__builtin_assume_aligned(tail + 8 * e, 8));
        rt = *reinterpret_cast<const int2*>(__builtin_assume_aligned(tail + 128 + 8 * e, 8));
      }
      __builtin_amdgcn_sched_barrier(0);
      stn_mfma3(xh[j & 1], xl[j & 1], bh, bl, acc0[j], acc1[j]);
      if (ABLATE != 1 && (j & 3) == 2 && j < 16) {    // a pair of tokens of the next piece, between this tile's MFMAs
        const int e = j >> 2;                         // pair e: tokens 8 q + 2 e, + 1
        unsigned hp, lp;
        float ps;
        ldw_form2(rx0, rx1, rn.x, rn.y, rt.x == col, rt.y == col, ps, hp, lp);
        if (e == 0) { nh.x = hp; nl.x = lp; zp = ps; } else if (e == 1) { nh.y = hp; nl.y = lp; zp += ps; }
        else if (e == 2) { nh.z = hp; nl.z = lp; zq = ps; } else { nh.w = hp; nl.w = lp; csum += live ? zp + (zq + ps) : 0.f; }
        stn_sched_pair();
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    bh = __builtin_bit_cast(f16x8, nh); bl = __builtin_bit_cast(f16x8, nl);
    cur = cur ? 0 : stn_xpiece(LDW_XKIB);
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
  for (int j = 0; j < STN_NT; ++j) {
    const int4 sv = *reinterpret_cast<const int4*>(shp + 16 * j);
    const int sh[4] = {sv.x, sv.y, sv.z, sv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      p.C[ldw_out_elem(by, p.slab, stn_out_row(j, q, i), p.V, col)] =
          stn_unscale(acc1[j][i], acc0[j][i], LDW_ES + sh[i]) * ce_sc;
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
  return (in_features == STN_N && V >= LDW_MIN_V && V % 32 == 0 && rows >= LDW_MIN_ROWS && rows % STN_KP == 0 &&
          rows < (1ll << 31) && (int64_t)STN_N * V < (1ll << 30)) ? 1 : 0;
}
int64_t pdn_outres_ce_dw_split_extra_bytes(int64_t rows) { return stn_extra_bytes(rows, LDW_XKIB); }

// slabs / colsum as pdn_outres_ce_dw_launch leaves them: range s (k_per_split tokens) at C + s * slab, colsum [ranges][V].
// `extra`: stn_extra_bytes(rows, LDW_XKIB) bytes, 16-byte aligned.
int pdn_outres_ce_dw_split_launch(const float* x, int64_t ldx, const float* logits, float* C, int V, int64_t rows,
                                  int64_t slab, int k_per_split, const float* lse, const int64_t* targets, float gscale,
                                  const float* gdev, float* colsum, void* extra, void* stream) {
  PDN_CHECK_ARG(pdn_outres_ce_dw_split_supported(rows, V, STN_N) && k_per_split > 0 && k_per_split % STN_KP == 0 &&
                    ((((uintptr_t)x | (uintptr_t)logits | (uintptr_t)extra) & 15) == 0) && (ldx & 3) == 0,
                "pdn_outres_ce_dw_split_launch: unsupported shape or alignment (rows %lld, V %d)", (long long)rows, V);
  static const int s_ablate = ls_env_switch("PDN_LMHEAD_DW_SPLIT_ABLATE", 0,
                                            "timing ablation active, dW and dbias of the split lm_head weight gradient are WRONG");
  const int M = (int)rows;
  LdwParams p;
  memset(&p, 0, sizeof(p));
  p.logits = logits; p.ximg = static_cast<const char*>(extra); p.xsh = stn_x_planes_launch(x, ldx, M, extra, lse, targets, stream);
  p.lse = lse; p.targets = targets; p.gdev = gdev; p.C = C; p.colsum = colsum;
  p.V = V; p.K = M; p.k_per_split = k_per_split; p.ldl = V; p.slab = slab; p.gscale = gscale;
  STN_LAUNCH_ABLATE(ldw_main_kernel, s_ablate, dim3((unsigned)((V + STN_COLS - 1) / STN_COLS), (unsigned)((M + k_per_split - 1) / k_per_split)),
                    stream, p);
  // slot 13 as well: "lm_head weight gradient with the CE gradient inside" is what bench.py asks for, whichever pipe ran it
  pdn_count(PDN_CNT_CE_DW);
  pdn_count(PDN_CNT_CE_DW_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
