// lm_head input gradient on split-fp16 MFMA at fp32 accuracy (gfx950 only):
//
//   dx[t] = gscale * ( sum_v e[t][v] W[:, v] / Z[t]  -  W[:, target[t]] ),   e = exp(logit - rowmax),  Z = sum_v e,
//   lse[t] = rowmax[t] + log Z[t]
//
// the contract of pdn_linear_ce_dx_deferred_f32 (csrc/gemm_outres.hip, CE == 2: `grad @ W^T` of pydynet/core/tensor.py:670
// behind the cross entropy of nn/functional.py:364-381, the softmax denominator found on the way), for the many-row
// shapes of a training step.  The product  u[t][d] = sum_v e[t][v] W[d][v]  is formed from fp16 operands like the forward
// (csrc/lm_head_split.hip):
//
//   e 2^15 = eh + el / 2048                       formed ON THE FLY from the fp32 logits, Z from the unsplit fp32 e
//   W[d][:] 2^s(d) = wh + wl / 2048               one pass per call, one power of two per OUTPUT COLUMN d
//   u 2^(15 + s(d)) = eh wh + (eh wl + el wh) / 2048
//
// The scale of e is 2^15 and not the forward's 2^8: e lies in (0, 1] with thousands of small terms per row, and whatever is
// below 2^-14 after scaling is an fp16 subnormal; at 2^15 the planes do not depend on how `cvt` or the matrix pipe treat
// those (tests/test_lm_head_dx_split_cpu.py), the largest plane value is 2^15, the largest residual 2^15.
//
// Structure: output-resident like gemm_outres_kernel.  A wave owns SIXTEEN rows and all 288 output columns of them, on
// `v_mfma_f32_16x16x32_f16`: 18 tiles x 4 registers x 2 sums (eh wh | eh wl + el wh) = 144 accumulators, two waves per
// SIMD, eight waves = 128 rows per workgroup.  The accumulators are transposed (W's tile is the MFMA A operand, e the B
// operand): a lane owns ONE row t = lane & 15 and four consecutive columns per tile, so Z, 1 / Z and the target are
// per-lane scalars and the store is 16 bytes wide.
// Everything the loop fetches arrives by LDS-DMA (`global_load_lds_dwordx4`), so no register is spent on data in flight:
//   * W's planes as 36 KiB images in LDS order (written by the W pass), two slots shared by the workgroup;
//   * the logits, read exactly once, into a ring of four 2 KiB pieces PRIVATE to the wave: an instruction fetches eight
//     rows x 128 bytes, eight lanes per 128-byte line; the 16-byte chunks of a row are XOR-swizzled on the source side so
//     that the ds_read_b128 by which lane (t, q) fetches its eight logits is conflict free.
// The DMA is issued from inline assembly: through the builtin the compiler takes every such instruction for a flat access
// that may touch LDS and from then on answers each dependency on a load OR an LDS read with a wait for all of them (the
// MFMA operand reads were serialised).  Per piece a wave issues W's piece s + 1 (five instructions) and THEN the logits
// of piece s + 4 (two); loads retire in order, so the one `s_waitcnt vmcnt(2)` in front of the piece's barrier means
// "W's piece s has landed" and, with it, everything older: the logits of piece s + 2 and before.  Three pieces of logits
// stay in flight and are never waited for earlier than two pieces after their issue.
// Deterministic: fixed order, no atomics.
#include "split_tn.h"
#include "gemm_prof.h"

#define LD_N 288                          // output columns: 18 tiles of 16
#define LD_NT 18
#define LD_KP 32                          // vocabulary entries per piece = one MFMA k-step
#define LD_PLANE (LD_N * LD_KP * 2)       // bytes of one fp16 plane of a piece: [d][4 units of 8 halves]
#define LD_PIECE (2 * LD_PLANE)           // 36 KiB: plane h, plane l
#define LD_RAW 2048                       // a wave's 16 rows x 32 logits of one piece
#define LD_RING 4                         // pieces of logits per wave in LDS
#define LD_ES 15                          // e is scaled by 2^15
#define LD_WG_ROWS 128
#define LD_MIN_ROWS (256 * LD_WG_ROWS)    // every CU gets a workgroup without cutting the vocabulary

// ---- W: the exponent of every output column d (a ROW of W as stored) ------------------------------------------------
__global__ __launch_bounds__(256) void ldx_w_shift_kernel(const float* __restrict__ w, int64_t ldw, int V, int* __restrict__ wsh) {
  __shared__ float sm[16];
  const float4* row = reinterpret_cast<const float4*>(w + (int64_t)blockIdx.x * ldw);
  float amax = 0.f;
  bool bad = false;
  for (int i = threadIdx.x; i < V / 4; i += 256) {
    const float4 v = row[i];
    const float f = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    amax = fmaxf(amax, f);
    bad |= !(fabsf(v.x) < INFINITY) || !(fabsf(v.y) < INFINITY) || !(fabsf(v.z) < INFINITY) || !(fabsf(v.w) < INFINITY);
  }
  amax = block_max(bad ? INFINITY : amax, sm);
  if (threadIdx.x == 0) wsh[blockIdx.x] = ls_shift(amax);
}

// ---- W: the plane images, one workgroup per piece of 32 vocabulary entries ------------------------------------------
// image of a piece: plane h, plane l; a plane is [d = 288][4 units of 16 bytes], unit q of row d (entries 8 q .. 8 q + 7 of
// the piece: what lane quarter q multiplies) at d * 4 + (q ^ ((d >> 2) & 3)): the sixteen rows x four units one
// ds_read_b128 fetches then cover every 16-byte slot of the banks four times, whichever sixteen lanes are served together.
__global__ __launch_bounds__(256) void ldx_split_w_kernel(const float* __restrict__ w, int64_t ldw, const int* __restrict__ wsh,
                                                           char* __restrict__ wimg) {
  char* img = wimg + (int64_t)blockIdx.x * LD_PIECE;
  const float* wp = w + (int64_t)blockIdx.x * LD_KP;
  for (int i = threadIdx.x; i < LD_N * 4; i += 256) {
    const int d = i >> 2, q = i & 3;
    const int sh = wsh[d];
    const float4 a = *reinterpret_cast<const float4*>(wp + (int64_t)d * ldw + 8 * q);
    const float4 b = *reinterpret_cast<const float4*>(wp + (int64_t)d * ldw + 8 * q + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    f16x8 hv, lv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      _Float16 h, l;
      ls_split(v[j], sh, h, l);
      hv[j] = h; lv[j] = l;
    }
    char* dst = img + (d * 4 + (q ^ ((d >> 2) & 3))) * 16;
    *reinterpret_cast<f16x8*>(dst) = hv;
    *reinterpret_cast<f16x8*>(dst + LD_PLANE) = lv;
  }
}

// ---- the product ----------------------------------------------------------------------------------------------------
struct LdxParams {
  const float* logits;
  const char* wimg;
  const int* wsh;
  const float* Wt;                // W^T (V x 288) fp32: the rows W[:, target] of the store
  const float* rowmax;
  const int64_t* targets;
  float* dx;
  float* lse;
  int M, V, np, max_parts;
  int64_t ldl, ldc;
  float gscale;
};

// two logits of the row: e = exp(logit - max), their sum for Z, their planes at 2^15 as two packed halves each.
// The empty asm pins the pair where it is written: the compiler otherwise collects the splits of a whole piece behind its
// last MFMA, a VALU phase of its own in which both waves of a SIMD leave the matrix pipe idle.
__device__ __forceinline__ void ldx_form2(float x0, float x1, float c2, float& esum, unsigned& hp, unsigned& lp) {
  const float e0 = __builtin_amdgcn_exp2f(fmaf(x0, 1.4426950408889634f, c2));
  const float e1 = __builtin_amdgcn_exp2f(fmaf(x1, 1.4426950408889634f, c2));
  esum = e0 + e1;
  f16x2 h, l;
  _Float16 a, b;
  ls_split_scaled(e0 * (float)(1 << LD_ES), a, b);
  h[0] = a; l[0] = b;
  ls_split_scaled(e1 * (float)(1 << LD_ES), a, b);
  h[1] = a; l[1] = b;
  hp = __builtin_bit_cast(unsigned, h);
  lp = __builtin_bit_cast(unsigned, l);
  asm volatile("" : "+v"(hp), "+v"(lp));
}

// ABLATE (timing experiments, PDN_LMHEAD_DX_SPLIT_ABLATE; the results are WRONG): 1 = the planes of e are constants, the
// logits are never read (MFMA + LDS only); 2 = the logits are fetched once, before the loop (no HBM stream).
template <int ABLATE>
__global__ __launch_bounds__(512, 1) void ldx_main_kernel(LdxParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[2 * LD_PIECE + 8 * LD_RING * LD_RAW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int row = blockIdx.x * LD_WG_ROWS + wave * 16 + r;
  const int np = p.np;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  // W: DMA instruction I (0..35) of a piece copies bytes 1024 I + 16 lane of its image; wave w issues I = w, w + 8, ..
  // (five each: the last four waves repeat instruction 35, so that every wave counts the same memory operations)
  const char* wsrc = p.wimg + lane * 16;
  auto dma_w = [&](int piece, int slot) __attribute__((always_inline)) {
    const char* src = wsrc + (int64_t)piece * LD_PIECE;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const int I = min(e * 8 + wave, 35);
      split_dma16(src + I * 1024, __builtin_amdgcn_readfirstlane(lds0 + slot + I * 1024));
    }
  };
  // logits: instruction i (0, 1) fetches rows 8 i .. 8 i + 7 of the wave's sixteen, lane l the 16-byte chunk at POSITION
  // l & 7 of row 8 i + (l >> 3), which holds chunk (l & 7) ^ ((row >> 1) & 7) of the row's 128 bytes
  // (rows past the end: the last row's logits, nothing stored)
  const int rw_base = 2 * LD_PIECE + wave * (LD_RING * LD_RAW);
  const float* lsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rr = 8 * i + (lane >> 3);
    const int grow = min(blockIdx.x * LD_WG_ROWS + wave * 16 + rr, p.M - 1);
    lsrc[i] = p.logits + (int64_t)grow * p.ldl + 4 * ((lane & 7) ^ ((rr >> 1) & 7));
  }
  auto dma_raw = [&](int piece, int ring) __attribute__((always_inline)) {
    const int64_t o = (int64_t)min(piece, np - 1) * LD_KP;     // (behind the last piece: a repeated fetch, never split)
    split_dma16(lsrc[0] + o, __builtin_amdgcn_readfirstlane(lds0 + rw_base + ring * LD_RAW));
    split_dma16(lsrc[1] + o, __builtin_amdgcn_readfirstlane(lds0 + rw_base + ring * LD_RAW + 1024));
  };
  // lane (t, q) reads logits 8 q .. 8 q + 7 of row t: chunks 2 q and 2 q + 1, at positions (2 q) ^ f and that ^ 1
  const int raw_lane = rw_base + r * 128 + (((2 * q) ^ ((r >> 1) & 7)) << 4);

  const int rowc = min(row, p.M - 1);
  float m = p.rowmax[rowc];
  for (int i = 1; i < p.max_parts; ++i) m = fmaxf(m, p.rowmax[(int64_t)i * p.M + rowc]);
  const float c2 = -m * 1.4426950408889634f;
  // this lane's share of the row's sum of exponentials, in three levels: the eight values of a piece as a tree, sixteen
  // pieces into zl, zl into zh -- a lane adds 8000 terms at V = 32000, and one running fp32 sum of those was 3e-6 of Z off
  // in the worst of 65536 rows (five units in the last place of lse)
  float zl = 0.f, zh = 0.f;

  // ---- prologue: piece 0 of W, pieces 0 .. 3 of the logits, the planes of piece 0 ------------------------------------
  dma_w(0, 0);
  if (ABLATE != 1) { dma_raw(0, 0); dma_raw(1, 1); dma_raw(2, 2); dma_raw(3, 3); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f16x8 bh, bl;
#pragma unroll
  for (int j = 0; j < 8; ++j) { bh[j] = (_Float16)1.f; bl[j] = (_Float16)0.5f; }
  if (ABLATE != 1) {
    const float4 v0 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + raw_lane, 16));
    const float4 v1 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + (raw_lane ^ 16), 16));
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    float s0, s1, s2, s3;
    ldx_form2(v0.x, v0.y, c2, s0, h0, l0);
    ldx_form2(v0.z, v0.w, c2, s1, h1, l1);
    ldx_form2(v1.x, v1.y, c2, s2, h2, l2);
    ldx_form2(v1.z, v1.w, c2, s3, h3, l3);
    zl = (s0 + s1) + (s2 + s3);
    const u32x4 hw = {h0, h1, h2, h3}, lw = {l0, l1, l2, l3};
    bh = __builtin_bit_cast(f16x8, hw); bl = __builtin_bit_cast(f16x8, lw);
  } else {
    zl = 1.f;
  }

  f32x4 acc0[LD_NT], acc1[LD_NT];
#pragma unroll
  for (int j = 0; j < LD_NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc0[j][i] = 0.f; acc1[j][i] = 0.f; }

  // fragment of tile j: row d = 16 j + r of the image, unit q: 1024 j bytes beside the lane's base
  const int frag = (r * 4 + (q ^ ((r >> 2) & 3))) * 16;
  constexpr int TOPWAIT = ABLATE == 0 ? 2 : 0;      // memory operations a wave issues per piece behind W's

  // ---- the pieces: 18 tiles of 3 MFMAs out of slot `cur`; in their shadow W's piece s + 1 is sent to the other slot
  // (every wave is past this piece's barrier, so nobody reads that slot any more), the logits of piece s + 4 are sent for
  // (into the ring slot whose piece s became planes while piece s - 1 ran) and those of piece s + 1 become planes ---------
  int cur = 0;
  for (int s = 0; s < np; ++s) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TOPWAIT) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const char* fb = smem + cur + frag;
    const float c2s = s + 1 < np ? c2 : -INFINITY;    // (behind the last piece: a repeated piece that must not reach Z)
    f16x8 wh[2], wl[2];
    u32x4 nh = __builtin_bit_cast(u32x4, bh), nl = __builtin_bit_cast(u32x4, bl);
    float4 rv0 = make_float4(0.f, 0.f, 0.f, 0.f), rv1 = rv0;
    float zp = 0.f, zq = 0.f;
#define LD_LOADW(X, J)                                                                                  \
  {                                                                                                     \
    wh[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024, 16));             \
    wl[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024 + LD_PLANE, 16));  \
  }
    LD_LOADW(0, 0)
#pragma unroll
    for (int j = 0; j < LD_NT; ++j) {
      if (j + 1 < LD_NT) { LD_LOADW((j + 1) & 1, j + 1) }
      if (j == 0) {
        dma_w(min(s + 1, np - 1), LD_PIECE - cur);
        if (ABLATE == 0) dma_raw(s + 4, s & (LD_RING - 1));
        if (ABLATE != 1) {
          const int ro = raw_lane + ((s + 1) & (LD_RING - 1)) * LD_RAW;
          rv0 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + ro, 16));
          rv1 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + (ro ^ 16), 16));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j & 1], bh, acc0[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j & 1], bh, acc1[j], 0, 0, 0);
      acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j & 1], bl, acc1[j], 0, 0, 0);
      if (ABLATE != 1 && (j & 3) == 2 && j < 16) {    // a pair of logits of the next piece, between this tile's MFMAs
        const int e = j >> 2;                         // pair e: values 2 e, 2 e + 1 of the lane's eight
        const float4 rv = (e >> 1) ? rv1 : rv0;
        unsigned hp, lp;
        float ps;
        ldx_form2((e & 1) ? rv.z : rv.x, (e & 1) ? rv.w : rv.y, c2s, ps, hp, lp);
        if (e == 0) { nh.x = hp; nl.x = lp; zp = ps; } else if (e == 1) { nh.y = hp; nl.y = lp; zp += ps; }
        else if (e == 2) { nh.z = hp; nl.z = lp; zq = ps; } else { nh.w = hp; nl.w = lp; zl += zp + (zq + ps); }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#undef LD_LOADW
    bh = __builtin_bit_cast(f16x8, nh); bl = __builtin_bit_cast(f16x8, nl);
    cur = LD_PIECE - cur;
    const bool flush = (s & 15) == 15;
    zh += flush ? zl : 0.f;
    zl = flush ? 0.f : zl;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the repeated last fetches must not outlive the workgroup's LDS

  // ---- rows: the lane's row t, columns 16 j + 4 q .. + 3 of tile j ----------------------------------------------------
  zl += zh;
  float z = zl + __shfl_xor(zl, 16, 64);
  z += __shfl_xor(z, 32, 64);
  if (row >= p.M) return;
  const float iz = 1.f / z;
  const int tg = min(max((int)p.targets[row], 0), p.V - 1);   // (an out-of-range target is reported by the loss kernel)
  if (q == 0) p.lse[row] = m + __logf(z);
  float* __restrict__ out = p.dx + (int64_t)row * p.ldc + 4 * q;
  const float* __restrict__ wt = p.Wt + (int64_t)tg * LD_N + 4 * q;
  const int* __restrict__ shp = p.wsh + 4 * q;
  const float sc = p.gscale;
#pragma unroll
  for (int j = 0; j < LD_NT; ++j) {
    const int4 sv = *reinterpret_cast<const int4*>(shp + 16 * j);
    const float4 w4 = *reinterpret_cast<const float4*>(wt + 16 * j);
    float4 o;
    o.x = sc * (ldexpf(fmaf(acc1[j][0], 1.f / 2048.f, acc0[j][0]), -(LD_ES + sv.x)) * iz - w4.x);
    o.y = sc * (ldexpf(fmaf(acc1[j][1], 1.f / 2048.f, acc0[j][1]), -(LD_ES + sv.y)) * iz - w4.y);
    o.z = sc * (ldexpf(fmaf(acc1[j][2], 1.f / 2048.f, acc0[j][2]), -(LD_ES + sv.z)) * iz - w4.z);
    o.w = sc * (ldexpf(fmaf(acc1[j][3], 1.f / 2048.f, acc0[j][3]), -(LD_ES + sv.w)) * iz - w4.w);
    *reinterpret_cast<float4*>(out + 16 * j) = o;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
int pdn_outres_wt_transpose_launch(const float* W, int64_t ldw, int V, float* Wt, void* stream);   // csrc/gemm_outres.hip

// PDN_LMHEAD_DX_SPLIT=0: the fp32 kernel at every size (A/B switch; read once, announced)
extern "C" int pdn_linear_ce_dx_deferred_split_supported(int64_t M, int V, int K) {
  static const int s_on = ls_env_switch("PDN_LMHEAD_DX_SPLIT", 1, "the lm_head input gradient stays on the fp32 MFMA kernel");
  return (s_on && K == LD_N && V >= LD_KP && V % LD_KP == 0 && (int64_t)LD_N * V < (1ll << 30) && M >= LD_MIN_ROWS &&
          M < (1ll << 31) - LD_WG_ROWS) ? 1 : 0;
}
// workspace: [W^T fp32: V x 288 | plane images: V / 32 pieces | 288 exponents]
extern "C" int64_t pdn_linear_ce_dx_deferred_split_workspace_bytes(int64_t M, int V, int K) {
  if (!pdn_linear_ce_dx_deferred_split_supported(M, V, K)) return 0;
  return (int64_t)V * LD_N * 4 + (int64_t)(V / LD_KP) * LD_PIECE + LD_N * 4;
}
extern "C" int pdn_linear_ce_dx_deferred_split_f32(const float* logits, const float* rowmax, int max_parts,
                                                   const int64_t* targets, float gscale, const float* W, float* dx, float* lse,
                                                   int64_t rows, int V, int in_features, void* workspace,
                                                   int64_t workspace_bytes, void* stream) {
  if (rows == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && rowmax && targets && W && dx && lse && workspace && max_parts >= 1,
                "pdn_linear_ce_dx_deferred_split_f32: null operand");
  if (!pdn_linear_ce_dx_deferred_split_supported(rows, V, in_features)) {
    pdn_set_error("pdn_linear_ce_dx_deferred_split_f32: unsupported shape rows=%lld V=%d in=%d", (long long)rows, V, in_features);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG(((((uintptr_t)logits | (uintptr_t)W | (uintptr_t)dx | (uintptr_t)workspace) & 15) == 0),
                "pdn_linear_ce_dx_deferred_split_f32: 16-byte alignment required");
  if (workspace_bytes < pdn_linear_ce_dx_deferred_split_workspace_bytes(rows, V, in_features)) {
    pdn_set_error("pdn_linear_ce_dx_deferred_split_f32: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                  (long long)pdn_linear_ce_dx_deferred_split_workspace_bytes(rows, V, in_features));
    return PDN_EWORKSPACE;
  }
  static const int s_ablate = ls_env_switch("PDN_LMHEAD_DX_SPLIT_ABLATE", 0,
                                            "timing ablation active, dx and lse of the split lm_head input gradient are WRONG");
  const int M = (int)rows, np = V / LD_KP;
  float* Wt = static_cast<float*>(workspace);
  char* wimg = reinterpret_cast<char*>(Wt + (int64_t)V * LD_N);
  int* wsh = reinterpret_cast<int*>(wimg + (int64_t)np * LD_PIECE);
  hipStream_t st = (hipStream_t)stream;
  const int tk = pdn_gemm_prof_begin(3, 2.0 * (double)rows * (double)V * (double)in_features, 0.0, stream);
  int rc = pdn_outres_wt_transpose_launch(W, V, V, Wt, stream);
  if (rc == PDN_OK) {
    hipLaunchKernelGGL(ldx_w_shift_kernel, dim3(LD_N), dim3(256), 0, st, W, (int64_t)V, V, wsh);
    hipLaunchKernelGGL(ldx_split_w_kernel, dim3(np), dim3(256), 0, st, W, (int64_t)V, wsh, wimg);
    LdxParams p;
    memset(&p, 0, sizeof(p));
    p.logits = logits; p.wimg = wimg; p.wsh = wsh; p.Wt = Wt; p.rowmax = rowmax; p.targets = targets;
    p.dx = dx; p.lse = lse; p.M = M; p.V = V; p.np = np; p.max_parts = max_parts;
    p.ldl = V; p.ldc = in_features; p.gscale = gscale;
    const dim3 grid((unsigned)((M + LD_WG_ROWS - 1) / LD_WG_ROWS)), block(512);
    if (s_ablate == 1) hipLaunchKernelGGL(ldx_main_kernel<1>, grid, block, 0, st, p);
    else if (s_ablate == 2) hipLaunchKernelGGL(ldx_main_kernel<2>, grid, block, 0, st, p);
    else hipLaunchKernelGGL(ldx_main_kernel<0>, grid, block, 0, st, p);
  }
  pdn_gemm_prof_end(tk, stream);
  if (rc != PDN_OK) return rc;
  // slot 12 as well: "lm_head input gradient + sum of exponentials" is what bench.py asks for, whichever pipe ran it
  pdn_count(PDN_CNT_CE_DX_DEFERRED);
  pdn_count(PDN_CNT_CE_DX_SPLIT);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
