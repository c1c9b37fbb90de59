// lm_head forward on split-fp16 MFMA at fp32 accuracy (gfx950 only):
//
//   logits (M x V) = x (M x 288) W (288 x V) + bias,   rowmax[m] = max_v logits[m][v]
//
// the contract of pdn_linear_rowmax_fwd_f32 (csrc/gemm_rowres.hip; `x @ W` of pydynet/core/tensor.py:657-676 in front of
// the cross entropy of nn/functional.py:364-381), for the many-row shapes of a training step.  On gfx950 the fp32-input
// MFMA runs at 1/16 of the f16 rate, so the product is formed from fp16 operands instead:
//
//   a * 2^s = h + l / 2048,   h = fp16(a * 2^s),  l = fp16((a * 2^s - h) * 2048)        (22 significant bits)
//   x w * 2^(sx + sw) = xh wh + (xh wl + xl wh) / 2048      (+ xl wl / 2^22: dropped, below fp32 round-off)
//
// with ONE power of two per row of x and per column of W that puts the row's / column's largest magnitude into
// [2^8, 2^9): fp16's narrow exponent never sees the data's scale, the products of two fp16 values are exact in the fp32
// accumulator, and the scale is removed exactly (v_ldexp with the SUM of the two integer exponents: no intermediate can
// overflow or underflow where the fp32 result would not).  Three f16 MFMAs replace sixteen MFMA-cycles' worth of fp32.
//
// Three launches (every address they form: csrc/lm_head_split_index.h, walked on the host by
// tests/lm_head_split_m16_check.cpp):
//   ls_split_x_kernel   one wave per row: exponent, the two fp16 planes in the order the product's fragments are loaded
//   ls_split_w_kernel   one workgroup per 32 columns: exponents, the planes TRANSPOSED ([column][k], k contiguous) as the
//                       image the product kernel copies to LDS, followed by the columns' exponents and bias.  Every call:
//                       the optimiser changes W every step and nothing tells the library when it did not.
//   ls_main_kernel      an N-sweep with resident A like csrc/gemm_rowtile.hip on `v_mfma_f32_16x16x32_f16`: a wave owns 32
//                       rows of x as two 16-row B fragments per k-step of 32 (both planes, 144 VGPRs, loaded once) and
//                       walks over the 32-column tiles of W; a tile is 18 phases (k-step, column half) of six MFMAs, each
//                       W fragment read from LDS feeding the six; the tile before leaves in the shadow of the MFMAs
//                       (slots between the phases, pinned with sched_barrier like the drain steps of csrc/gemm_rowtile.hip).
// The accumulators are TRANSPOSED (W tile as the A operand, x rows as the B operand): lane (r, q) owns rows r and 16 + r of
// the wave's 32 and, per column half, four consecutive columns, so the scale of a row is one register, its maximum a
// running maximum in ONE register (two exchanges between the lane quarters at the end) and the columns' exponents / bias
// are two broadcast 16-byte LDS reads per group.
// W's tile arrives by LDS-DMA (`split_dma16`, csrc/split_tn.h) issued from inline assembly at the start of the tile
// before: no register holds data in flight and nothing is written to LDS by the waves but the leaving tile.  The one wait
// is written out: memory operations retire in order, so `s_waitcnt vmcnt(4)` at the end of a tile -- behind its DMA come
// exactly the four row-wise stores of the tile before -- means "the next image has landed".  Where the stores may be
// skipped (the first tile, GUARD, the ablation) the wait is vmcnt(0).
// The store: a lane's 16 bytes of 16 different rows per instruction would write sixteen cache lines an eighth each (the
// first version of this kernel spent 3.1 ms of 9.3 in such stores).  The finished tile therefore passes through a 4.5 KiB
// LDS area private to the wave and leaves ROW-wise -- eight lanes write one whole 128-byte line.
// Deterministic: fixed order, no atomics.
#include "split_tn.h"
#include "lm_head_split_index.h"
#include "gemm_prof.h"
#include <stdlib.h>
#include <type_traits>

// (switches, ls_shift, ls_split: lm_head_split.h.  PDN_LMHEAD_SPLIT_ABLATE, tools/lmhead_probe.py: a non-zero value makes
// the kernel skip its stores, i.e. the logits are WRONG.)

// ---- x: one wave per row ------------------------------------------------------------------------------------------
// rows M .. Mpad - 1 (Mpad: a multiple of 256) are written as zeros, so that every wave of the product kernel loads
// initialised fragments.  Lane u < 36 holds unit u of the row: k = 8 u .. 8 u + 7.
__global__ __launch_bounds__(256) void ls_split_x_kernel(const float* __restrict__ x, int64_t ldx, int M,
                                                          char* __restrict__ ximg, int* __restrict__ nex) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  if (lane < LS_UNITS && row < M) {
    const float4* src = reinterpret_cast<const float4*>(x + (int64_t)row * ldx + 8 * lane);
    const float4 a = src[0], b = src[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  float amax = 0.f;
  bool bad = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = fabsf(v[j]);
    amax = fmaxf(amax, f);
    bad |= !(f < INFINITY);                         // Inf or NaN (fmaxf alone would drop a NaN)
  }
  amax = wave_max(amax);
  if (__any(bad ? 1 : 0)) amax = INFINITY;
  const int sh = ls_shift(amax);
  if (lane < LS_UNITS) {
    f16x8 hv, lv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      _Float16 h, l;
      ls_split(v[j], sh, h, l);
      hv[j] = h; lv[j] = l;
    }
    char* dst = ximg + (int64_t)(row >> 5) * LS_XBLK + ls_x_unit(row & 31, lane);
    *reinterpret_cast<f16x8*>(dst) = hv;
    *reinterpret_cast<f16x8*>(dst + LS_XBLK / 2) = lv;
  }
  if (lane == 0) nex[row] = -sh;
}

// ---- W: one workgroup per 32-column tile --------------------------------------------------------------------------
// image of a tile: plane h, plane l ([n = 32][36 units of 8 k], unit u of column n at ls_w_unit(n, u)), 32 negated
// exponents, 32 bias values.
__global__ __launch_bounds__(256) void ls_split_w_kernel(const float* __restrict__ w, int64_t ldw,
                                                          const float* __restrict__ bias, char* __restrict__ wimg) {
  __shared__ float sm[LS_K * 33];
  __shared__ float smax[8 * 32];
  const int tid = threadIdx.x, c = tid & 31, kq = tid >> 5, v0 = blockIdx.x * 32;
  float amax = 0.f;
  bool bad = false;
  for (int k = kq; k < LS_K; k += 8) {
    const float f = w[(int64_t)k * ldw + v0 + c];
    sm[k * 33 + c] = f;
    amax = fmaxf(amax, fabsf(f));
    bad |= !(fabsf(f) < INFINITY);
  }
  smax[kq * 32 + c] = bad ? INFINITY : amax;
  __syncthreads();
  char* tile = wimg + (int64_t)blockIdx.x * LS_TILE;
  float cm = smax[c];
#pragma unroll
  for (int i = 1; i < 8; ++i) cm = fmaxf(cm, smax[i * 32 + c]);
  const int sh = ls_shift(cm);                      // (column c: the same for every unit this thread writes)
  for (int u = tid; u < 32 * LS_UNITS; u += 256) {  // u = 32 ku + n: n == c
    const int ku = u >> 5;
    f16x8 hv, lv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      _Float16 h, l;
      ls_split(sm[(8 * ku + j) * 33 + c], sh, h, l);
      hv[j] = h; lv[j] = l;
    }
    char* dst = tile + ls_w_unit(c, ku);
    *reinterpret_cast<f16x8*>(dst) = hv;
    *reinterpret_cast<f16x8*>(dst + LS_PLANE) = lv;
  }
  if (tid < 32) {
    reinterpret_cast<int*>(tile + LS_TAIL)[tid] = -sh;
    reinterpret_cast<float*>(tile + LS_TAIL + 128)[tid] = bias ? bias[v0 + tid] : 0.f;
  }
}

// ---- the product ------------------------------------------------------------------------------------------------
struct LsParams {
  const char* ximg;
  const int* nex;
  const char* wimg;
  float* C;
  float* rowmax;
  int M;
  unsigned ldl;
  int ntiles, tpw;                // tiles in total / per workgroup (grid.y)
};

template <int V> using ls_ic = std::integral_constant<int, V>;

// GUARD: M is not a multiple of 256 (row test in every store).  ABLATE (PDN_LMHEAD_SPLIT_ABLATE, timing experiments; the
// logits are WRONG): 1 = no stores.
// LDS: a ring of THREE slots.  During tile t the waves multiply out of slot t % 3, the DMA fills slot (t + 1) % 3 and
// the exponents / bias of tile t - 1 (which leaves meanwhile) are read from slot (t - 1) % 3: one barrier per tile orders
// all three.
template <bool GUARD, int ABLATE>
__global__ __launch_bounds__(512, 1) void ls_main_kernel(LsParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[LS_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int blk = blockIdx.x * 8 + wave, m0 = blk * 32;
  const int T0 = blockIdx.y * p.tpw;
  const int T1 = min(p.ntiles, T0 + p.tpw);
  if (T0 >= T1) return;                             // (the whole workgroup)
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  // staging: 37 DMA instructions per image, five or four per wave (the last one: sixteen lanes)
  const char* wsrc = p.wimg + lane * 16;
  auto dma_tile = [&](int t, int slot) __attribute__((always_inline)) {
    const char* src = wsrc + (int64_t)t * LS_TILE;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int I = ls_dma_instr(wave, e);
      split_dma16(src + I * 1024, __builtin_amdgcn_readfirstlane(lds0 + slot + I * 1024));
    }
    if (ls_dma_count(wave) == 5) {
      const int I = ls_dma_instr(wave, 4);
      if (lane < ls_dma_lanes(I)) split_dma16(src + I * 1024, __builtin_amdgcn_readfirstlane(lds0 + slot + I * 1024));
    }
  };

  // ---- prologue: the first tile into slot 0, the wave's 32 rows (both planes) into registers --------------------
  dma_tile(T0, 0);
  f16x8 xh[LS_KS][2], xl[LS_KS][2];
  {
    const char* xp = p.ximg + (int64_t)blk * LS_XBLK;
#pragma unroll
    for (int s = 0; s < LS_KS; ++s)
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        xh[s][rb] = *reinterpret_cast<const f16x8*>(xp + ls_x_frag(s, rb, lane));
        xl[s][rb] = *reinterpret_cast<const f16x8*>(xp + LS_XBLK / 2 + ls_x_frag(s, rb, lane));
      }
  }
  // (rows up to the next multiple of 256 exist in the workspace)
  const int nexv[2] = {p.nex[m0 + r], p.nex[m0 + 16 + r]};
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  f32x4 acc0[2][2], acc1[2][2];                     // [column half c][row half rb]
  float out[16];                                    // the tile that leaves: acc0 + acc1 / 2048, still scaled; group g = 2 c + rb
#pragma unroll
  for (int i = 0; i < 16; ++i) out[i] = 0.f;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  float mx[2] = {-INFINITY, -INFINITY};

  const int frag = ls_w_frag_lane(lane);
  // The leaving tile goes through a private LDS area of the wave and is stored ROW-wise: a lane owns two rows in the
  // accumulators (16 bytes of one per group), but eight lanes that store 16 bytes each of ONE row write a whole 128-byte
  // line, where 16 lanes storing to 16 rows write 16 lines an eighth each.
  char* stg = smem + 3 * LS_SLOT + wave * LS_STG;
  const int srow = m0 + ls_store_row(0, lane);
  const unsigned ob = 4u * (unsigned)ls_store_row(0, lane) * p.ldl + 4u * (unsigned)ls_store_col(lane);   // BYTES beside a wave-uniform base
  const unsigned ldl32 = 32u * p.ldl;               // eight rows, in bytes

  // group g of the leaving tile: scale removed, bias, maximum
  auto drain_group = [&](int g, const int4& ne, const float4& bv) __attribute__((always_inline)) {
    const int e = nexv[g & 1];
    float4 o;
    o.x = ldexpf(out[4 * g + 0], e + ne.x) + bv.x;
    o.y = ldexpf(out[4 * g + 1], e + ne.y) + bv.y;
    o.z = ldexpf(out[4 * g + 2], e + ne.z) + bv.z;
    o.w = ldexpf(out[4 * g + 3], e + ne.w) + bv.w;
    mx[g & 1] = fmaxf(fmaxf(mx[g & 1], fmaxf(o.x, o.y)), fmaxf(o.z, o.w));
    *reinterpret_cast<float4*>(__builtin_assume_aligned(stg + ls_stg_write(g, lane), 16)) = o;
  };
  // store j: rows 8 j .. 8 j + 7 of the tile, a 128-byte line per eight lanes
  auto store_rows = [&](int j, float* Cd) __attribute__((always_inline)) {
    const float4 v = *reinterpret_cast<const float4*>(__builtin_assume_aligned(stg + ls_stg_read(j, lane), 16));
    if (ABLATE != 1 && (!GUARD || srow + 8 * j < p.M))
      *reinterpret_cast<float4*>(reinterpret_cast<char*>(Cd) + ob + (unsigned)j * ldl32) = v;
  };

  // ---- one tile: 18 phases of 6 MFMAs out of slot `cur`; in their shadow tile t + 1 is sent for into `nxt` and tile
  // t - 1 leaves (its exponents and bias: slot `prv`) -----------------------------------------------------------
  auto run_tile = [&](auto firstc, int t, int cur, int prv, int nxt) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(firstc)::value != 0;
    lds_barrier();
    float* Cd = p.C + (int64_t)m0 * p.ldl + 32 * (t - 1);
    const char* fb = smem + cur + frag;
    const char* tp = smem + prv;
    f16x8 wh[2], wl[2];
    int4 ne = make_int4(0, 0, 0, 0);
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
#define LS_LOADW(X, P)                                                                              \
  {                                                                                                 \
    const char* f = fb + ls_w_frag_phase(P);                                                        \
    wh[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(f, 16));                       \
    wl[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(f + LS_PLANE, 16));            \
  }
    LS_LOADW(0, 0)
#pragma unroll
    for (int ph = 0; ph < LS_PH; ++ph) {
      const int c = ph & 1, s = ph >> 1;
      if (ph + 1 < LS_PH) { LS_LOADW((ph + 1) & 1, ph + 1) }
      const int dg = (ph & 1) && ph < 8 ? (ph >> 1) : -1;        // groups 0..3 leave for the LDS area in slots 1, 3, 5, 7
      if (!FIRST && dg >= 0) {
        ne = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tp + ls_tail_ne(dg >> 1, q), 16));
        bv = *reinterpret_cast<const float4*>(__builtin_assume_aligned(tp + ls_tail_ne(dg >> 1, q) + 128, 16));
      }
      __builtin_amdgcn_sched_barrier(0);
      acc0[c][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ph & 1], xh[s][0], s == 0 ? zero4 : acc0[c][0], 0, 0, 0);
      acc1[c][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ph & 1], xh[s][0], s == 0 ? zero4 : acc1[c][0], 0, 0, 0);
      acc0[c][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ph & 1], xh[s][1], s == 0 ? zero4 : acc0[c][1], 0, 0, 0);
      acc1[c][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[ph & 1], xh[s][1], s == 0 ? zero4 : acc1[c][1], 0, 0, 0);
      acc1[c][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ph & 1], xl[s][0], acc1[c][0], 0, 0, 0);
      acc1[c][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[ph & 1], xl[s][1], acc1[c][1], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      // ---- slot ph ----
      if (ph == 0 && t + 1 < T1) dma_tile(t + 1, nxt);
      if (!FIRST && dg >= 0) drain_group(dg, ne, bv);
      if (!FIRST && (ph & 1) && ph >= 9 && ph < 17) store_rows((ph - 9) >> 1, Cd);   // ... and for memory in slots 9, 11, 13, 15
      __builtin_amdgcn_sched_barrier(0);
    }
#undef LS_LOADW
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) out[4 * g + i] = fmaf(acc1[g >> 1][g & 1][i], 1.f / 2048.f, acc0[g >> 1][g & 1][i]);
    // the next image has landed: behind its DMA this wave issued the four stores, or nothing
    if (FIRST || GUARD || ABLATE != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  };

  int cur = 0, prv = 2 * LS_SLOT, nxt = LS_SLOT;
  run_tile(ls_ic<1>{}, T0, cur, prv, nxt);
  for (int t = T0 + 1; t < T1; ++t) {
    prv = cur; cur = nxt; nxt = nxt == 2 * LS_SLOT ? 0 : nxt + LS_SLOT;
    run_tile(ls_ic<0>{}, t, cur, prv, nxt);
  }
  // the last tile leaves with nothing to hide behind (its slot is not written again)
  {
    float* Cd = p.C + (int64_t)m0 * p.ldl + 32 * (T1 - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const char* tl = smem + cur + ls_tail_ne(g >> 1, q);
      const int4 ne = *reinterpret_cast<const int4*>(__builtin_assume_aligned(tl, 16));
      const float4 bv = *reinterpret_cast<const float4*>(__builtin_assume_aligned(tl + 128, 16));
      drain_group(g, ne, bv);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) store_rows(j, Cd);
  }
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    float m = fmaxf(mx[rb], __shfl_xor(mx[rb], 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const int row = m0 + 16 * rb + r;
    if (q == 0 && row < p.M) p.rowmax[(int64_t)blockIdx.y * p.M + row] = m;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------

// PDN_LMHEAD_SPLIT=0: the fp32 kernel at every size (A/B switch; read once, announced)
extern "C" int pdn_linear_rowmax_split_supported(int64_t M, int V, int K) {
  static const int s_on = ls_env_switch("PDN_LMHEAD_SPLIT", 1, "the lm_head forward stays on the fp32 MFMA kernel");
  return (s_on && K == LS_K && V >= 32 && V % 32 == 0 && V < (1 << 24) && M >= LS_MIN_ROWS && M < (1ll << 31) - 256) ? 1 : 0;
}
extern "C" int64_t pdn_linear_rowmax_split_workspace_bytes(int64_t M, int V, int K) {
  if (!pdn_linear_rowmax_split_supported(M, V, K)) return 0;
  return ls_workspace_bytes(M, V);
}
extern "C" int pdn_linear_rowmax_split_parts(int64_t M, int V, int K) {
  if (!pdn_linear_rowmax_split_supported(M, V, K)) return 0;
  return ls_plan_ranges(M, V);
}
extern "C" int pdn_linear_rowmax_split_fwd_f32(const float* x, const float* w, const float* bias, float* logits,
                                               float* rowmax, int M, int V, int K, int64_t ldx, int64_t ldw, int64_t ldl,
                                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (M == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(x && w && logits && rowmax && workspace, "pdn_linear_rowmax_split_fwd_f32: null operand");
  if (!pdn_linear_rowmax_split_supported(M, V, K) || (ldx & 3) || (ldl & 3) || ldx < K || ldw < V || ldl < V ||
      ldl >= (1 << 24) || (((uintptr_t)x | (uintptr_t)logits | (uintptr_t)workspace) & 15)) {
    pdn_set_error("pdn_linear_rowmax_split_fwd_f32: unsupported shape M=%d V=%d K=%d (or leading dimension / alignment)", M, V, K);
    return PDN_EUNSUPPORTED;
  }
  if (workspace_bytes < pdn_linear_rowmax_split_workspace_bytes(M, V, K)) {
    pdn_set_error("pdn_linear_rowmax_split_fwd_f32: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)pdn_linear_rowmax_split_workspace_bytes(M, V, K));
    return PDN_EWORKSPACE;
  }
  static const int s_ablate = ls_env_switch("PDN_LMHEAD_SPLIT_ABLATE", 0, "timing ablation active, the logits of the split lm_head kernel are WRONG");
  const int64_t mp = ls_mpad(M);
  const int nt = V / 32;
  char* wimg = static_cast<char*>(workspace);
  char* ximg = wimg + (int64_t)nt * LS_TILE;
  int* nex = reinterpret_cast<int*>(ximg + mp / 32 * LS_XBLK);
  hipStream_t st = (hipStream_t)stream;
  const int tk = pdn_gemm_prof_begin(2, 2.0 * M * (double)V * K, 0.0, stream);
  hipLaunchKernelGGL(ls_split_w_kernel, dim3(nt), dim3(256), 0, st, w, ldw, bias, wimg);
  hipLaunchKernelGGL(ls_split_x_kernel, dim3((unsigned)(mp / 4)), dim3(256), 0, st, x, ldx, M, ximg, nex);
  LsParams p;
  memset(&p, 0, sizeof(p));
  p.ximg = ximg; p.nex = nex; p.wimg = wimg; p.C = logits; p.rowmax = rowmax;
  p.M = M; p.ldl = (unsigned)ldl; p.ntiles = nt; p.tpw = ls_plan_tpw(M, V);
  const dim3 grid((unsigned)(mp / 256), ls_plan_ranges(M, V)), block(512);
  if (M % 256 != 0) {
    if (s_ablate) hipLaunchKernelGGL((ls_main_kernel<true, 1>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((ls_main_kernel<true, 0>), grid, block, 0, st, p);
  } else {
    if (s_ablate) hipLaunchKernelGGL((ls_main_kernel<false, 1>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((ls_main_kernel<false, 0>), grid, block, 0, st, p);
  }
  pdn_gemm_prof_end(tk, stream);
  // slot 5 as well: "vocabulary projection + row maxima" is what bench.py's batch gate asks for, whichever pipe ran it
  pdn_count(PDN_CNT_ROWTILE_ROWMAX);
  pdn_count(PDN_CNT_LMHEAD_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
