// Output-resident products on split-fp16 MFMA at fp32 accuracy (gfx950 only):
//
//   C (M x 288) = A (M x K) B + bias + residual
//
// for the many-row calls of a training step that csrc/gemm_outres.hip ran on the fp32 pipe: the layer input gradients
// dX = [dq | dk | dv] [Wq | Wk | Wv]^T and [dgate | dup] [Wg | Wu]^T (NT, the weights read as blocks where they live) and
// the down projection h W_down + residual (NN).  outres_launch routes here (pdn_outres_split_takes); there is no entry of
// its own.  pdn_gemm_f32 sends the 288 x 288 products here as well (K = 288, nine pieces: ctx Wo + x and dz Wo^T, csrc/gemm.hip).  The product is formed from fp16 operands like the lm_head input gradient (csrc/lm_head_dx_split.hip), whose
// main kernel this is without the exponential, Z, the targets and W^T:
//
//   B[:, d] 2^s(d) = wh + wl / 2048            one pass per call, one power of two per OUTPUT COLUMN d
//   A[t, :] 2^S(t) = ah + al / 2048            formed ON THE FLY, one RUNNING power of two per ROW t
//   C 2^(S(t) + s(d)) = ah wh + (ah wl + al wh) / 2048
//
// A has no bound and no pass of its own (that pass would cost most of the gain).  A lane owns one row (lane & 15) with the
// three other lanes lane >> 4; before a piece of 32 values is split the four take the largest finite magnitude of the
// row's 32 values (eight per lane, two cross-lane steps).  If that maximum times 2^S would reach 2^15, or S is not set
// yet, S is set so that the maximum lands in [2^12, 2^13), the piece is split with the new S and, once the MFMAs of the
// current piece are through, both accumulator sets of the lane are multiplied by the power of two between the old and the
// new S (under a wave-uniform "any lane moved" branch).  S only falls; all-zero pieces are ignored; non-finite values stay
// out of the maximum and come out non-finite in their row only.  The exponent is per ROW and not per wave because rows
// are tokens: neighbours may differ by many orders of magnitude (per-token loss weights, rows next to ignored ones), and a
// row 1e-9 below its group's maximum would fall into fp16 subnormals entirely.
//
// Structure: a wave owns SIXTEEN rows and all 288 columns on `v_mfma_f32_16x16x32_f16` (144 accumulators, transposed: W's
// tile is the MFMA A operand), eight waves = 128 rows per block, W's planes as 36 KiB images by LDS-DMA into two slots, A
// read exactly once by LDS-DMA through a ring of four pieces private to the wave (see csrc/lm_head_dx_split.hip for the
// DMA, its waits and the swizzles; csrc/outres_split_index.h has every index).  With 8 .. 128 pieces per block the first
// W piece, the ring fill and the store drain are no longer amortised over 1000 pieces, so the kernel is PERSISTENT: 256
// workgroups walk their blocks as one stream of pieces -- while the last pieces of a block run, W's piece 0 and the first
// four pieces of A of the NEXT block are fetched and its piece 0 is split, so a block's stores run with the next block's
// operands in LDS already.  Deterministic: fixed order, no atomics.
#include "split_tn.h"
#include "outres_split_index.h"
#include "gemm_routes.h"
#include "weight_images.h"

extern "C" int pdn_malloc(void** ptr, int64_t bytes);
extern "C" int pdn_free(void* ptr);

// ---- W: the largest magnitude per output column of every piece (Inf for a non-finite one).  The bodies are those of
// csrc/weight_images.h, shared with the batched builder. -----------------------------------------------------------------
template <bool NN>
__global__ __launch_bounds__(256) void ors_w_max_kernel(OrsWParams p) {
  __shared__ float tile[NN ? ORS_W_TILE : 1];
  if (NN) ors_w_stage_nn(p, tile, blockIdx.x, 0, ORS_N / 4);
  for (int i = threadIdx.x; i < ORS_N * 4; i += 256) {
    const int d = i >> 2, q = i & 3;
    float v[8];
    ors_w_unit<NN>(p, tile, blockIdx.x, d, q, v);
    float m = ors_w_max8(v);
    m = fmaxf(m, __shfl_xor(m, 1, 64));                     // the four units of a column lie in four adjacent lanes
    m = fmaxf(m, __shfl_xor(m, 2, 64));
    if (q == 0) p.pmax[(int64_t)blockIdx.x * ORS_N + d] = m;
  }
}

// ---- W: the plane images, ORS_IMG_WGS workgroups per piece -------------------------------------------------------------------------
template <bool NN>
__global__ __launch_bounds__(256) void ors_w_img_kernel(OrsWParams p) {
  __shared__ float tile[NN ? ORS_W_TILE : 1];
  if (NN) ors_w_stage_nn(p, tile, blockIdx.x, 0, ORS_N / 4);
  char* img = p.wimg + (int64_t)blockIdx.x * ORS_PIECE;
  // ONE unit per thread, the 1152 units of a piece over ORS_IMG_WGS workgroups (grid.y): with np workgroups of 4.5 units per
  // thread the pass was a chain of five memory round trips on a tenth of the chip (NN: every workgroup stages the whole tile)
  const int i = blockIdx.y * 256 + threadIdx.x;
  if (i < ORS_N * 4) {
    const int d = i >> 2, q = i & 3;
    float amax = 0.f;
    for (int s = 0; s < p.np; ++s) amax = fmaxf(amax, p.pmax[(int64_t)s * ORS_N + d]);
    const int sh = ls_shift(amax);
    if (blockIdx.x == 0 && q == 0) p.wsh[d] = sh;
    float v[8];
    ors_w_unit<NN>(p, tile, blockIdx.x, d, q, v);
    ors_w_put(img, d, q, sh, v);
  }
}

// ---- the product ----------------------------------------------------------------------------------------------------------
struct OrsParams {
  const float* A;
  const char* wimg;
  const int* wsh;
  const float* bias;              // may be null
  const float* residual;          // may be null; row stride ldc; may be C itself
  float* C;
  int M, np, nblk;
  int64_t lda, ldc;
  // epilogue 1 (the RMSNorm backward in the drain): C is dx; x, the held gradient and dx share the row stride ldc
  const float* nx;                // the norm's raw input
  const float* nw;                // its 288 weights
  const float* nrms;              // M values
  const float* nex;               // may be null: the gradient x already holds, added to dx
  float* dwpart;                  // may be null: gridDim.x x 288 partial sums of the weight gradient
};

// the sum over the sixteen lanes r = lane & 15 of a row of the wave, in every one of them and with the same bits in each
// (every step adds the same two numbers on both sides): two steps inside the quads, then the halves of eight and of sixteen
// mirrored onto each other.  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ float ors_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float ors_row16_sum(float v) {
  v = ors_dpp_add<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  v = ors_dpp_add<0x4E>(v);       // quad_perm [2, 3, 0, 1]
  v = ors_dpp_add<0x141>(v);      // row_half_mirror
  return ors_dpp_add<0x140>(v);   // row_mirror
}

// the largest finite magnitude of eight values
__device__ __forceinline__ float ors_max8(const float4& a, const float4& b) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float f = fabsf(v[j]);
    m = fmaxf(m, f < INFINITY ? f : 0.f);
  }
  return m;
}
__device__ __forceinline__ int ors_step_exp(float mx, int S) { return ors_next_exp(mx > 0.f, __builtin_amdgcn_frexp_expf(mx), S); }
// two values of the row at 2^S as two packed halves per plane (the empty asm pins the pair where it is written, see
// ldx_form2 of csrc/lm_head_dx_split.hip)
__device__ __forceinline__ void ors_form2(float x0, float x1, int S, unsigned& hp, unsigned& lp) {
  f16x2 h, l;
  _Float16 a, b;
  ls_split_scaled(ldexpf(x0, S), a, b);
  h[0] = a; l[0] = b;
  ls_split_scaled(ldexpf(x1, S), a, b);
  h[1] = a; l[1] = b;
  hp = __builtin_bit_cast(unsigned, h);
  lp = __builtin_bit_cast(unsigned, l);
  asm volatile("" : "+v"(hp), "+v"(lp));
}

// ABLATE (timing experiments, PDN_OUTRES_SPLIT_ABLATE; the results are WRONG): 1 = the planes of A are constants, A is
// never read (MFMA + LDS only); 2 = A is fetched once, before the loop (no HBM stream in); 3 = nothing is stored.
//
// EPI 1: the drain does not store C = dy but the RMSNorm backward of it (csrc/fused.hip: rmsnorm_bwd_kernel), per row t
//   z = x[t] / rms[t],  dz = dy w,  dx[t] = (dz - z mean(z dz)) / rms[t] (+ held gradient),  dw += dy z
// A row's 288 columns lie in the four lanes lane & 15, + 16, + 32, + 48.  Pass A forms dy tile by tile, reads x once (as
// the residual is requested in epilogue 0), adds up the row's dot product and the weight-gradient sums, and leaves dz and z
// IN THE TWO ACCUMULATOR SETS of the element, which are zeroed behind the drain anyway; pass B forms dx from them, so x is
// read once and dy never leaves the registers.  dw: a tile's float4 summed over the wave's sixteen rows, the r == 0 lanes
// add it into a row of LDS private to the wave, the eight rows are added in a fixed order into dwpart[workgroup] at the
// end (no atomics; csrc/fused.hip's colsum_partials_kernel sums the workgroups).
template <int ABLATE, int EPI = 0>
__global__ __launch_bounds__(512, 1) void ors_main_kernel(OrsParams p) {
  __shared__ __attribute__((aligned(1024))) char smem[ORS_LDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int np = p.np, nblk = p.nblk, grid = gridDim.x;
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
  constexpr bool STREAM = ABLATE == 0 || ABLATE == 3;
  // for the drain: the 288 column exponents and the bias (-0 where there is none: x + -0 is x bit for bit, -0 included).
  // Written here, read behind at least eight barriers.
  __shared__ __attribute__((aligned(16))) int col_sh[ORS_N];
  __shared__ __attribute__((aligned(16))) float col_bias[ORS_N];
  if (tid < ORS_N) { col_sh[tid] = p.wsh[tid]; col_bias[tid] = p.bias ? p.bias[tid] : -0.f; }
  // EPI 1: [the norm's 288 weights | eight rows of weight-gradient sums]; read behind the same barriers
  __shared__ __attribute__((aligned(16))) float norm_sh[EPI == 1 ? ORS_NORM_FLOATS : 1];
  if constexpr (EPI == 1) {
    if (tid < ORS_N) norm_sh[tid] = p.nw[tid];
    for (int i = tid; i < ORS_DW_FLOATS; i += 512) norm_sh[ORS_N + i] = 0.f;
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

  // W: the image of piece `piece` into slot `slot`, five instructions per wave
  const char* wsrc = p.wimg + lane * 16;
  auto dma_w = [&](int piece, int slot) __attribute__((always_inline)) {
    const char* src = wsrc + (int64_t)piece * ORS_PIECE;
#pragma unroll
    for (int e = 0; e < 5; ++e) {
      const int I = ors_wdma_instr(e, wave);
      split_dma16(src + I * 1024, __builtin_amdgcn_readfirstlane(lds0 + slot + I * 1024));
    }
  };
  // A: the two fetches of a piece of this block (`cur`) or of the workgroup's next one
  auto a_src = [&](int blk, int i) __attribute__((always_inline)) {
    return p.A + ors_a_row(blk, wave, ors_raw_row(i, lane), p.M) * p.lda + 4 * ors_raw_chunk(i, lane);
  };
  int blk = blockIdx.x, nxt = ors_next_block(blk, grid, nblk);
  const float* ac0 = a_src(blk, 0);
  const float* ac1 = a_src(blk, 1);
  const float* an0 = a_src(nxt, 0);
  const float* an1 = a_src(nxt, 1);
  const int rw_base = ORS_RING0 + wave * (ORS_RING * ORS_RAW);
  auto dma_raw = [&](const float* s0, const float* s1, int piece, int ring) __attribute__((always_inline)) {
    const int64_t o = (int64_t)piece * ORS_KP;
    split_dma16(s0 + o, __builtin_amdgcn_readfirstlane(lds0 + rw_base + ring * ORS_RAW));
    split_dma16(s1 + o, __builtin_amdgcn_readfirstlane(lds0 + rw_base + ring * ORS_RAW + 1024));
  };
  const int raw_lane = rw_base + ors_raw_lane(r, q);

  // ---- prologue: piece 0 of W, pieces 0 .. 3 of A, the planes of piece 0 -----------------------------------------------
  dma_w(0, 0);
  if (ABLATE != 1) { dma_raw(ac0, ac1, 0, 0); dma_raw(ac0, ac1, 1, 1); dma_raw(ac0, ac1, 2, 2); dma_raw(ac0, ac1, 3, 3); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f16x8 bh, bl;
#pragma unroll
  for (int j = 0; j < 8; ++j) { bh[j] = (_Float16)1.f; bl[j] = (_Float16)0.5f; }
  int S = ABLATE == 1 ? 0 : ORS_UNSET;          // the row's exponent (the same in the row's four lanes)
  if (ABLATE != 1) {
    const float4 v0 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + raw_lane, 16));
    const float4 v1 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + (raw_lane ^ 16), 16));
    float mx = ors_max8(v0, v1);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    S = ors_step_exp(mx, S);
    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
    ors_form2(v0.x, v0.y, S, h0, l0);
    ors_form2(v0.z, v0.w, S, h1, l1);
    ors_form2(v1.x, v1.y, S, h2, l2);
    ors_form2(v1.z, v1.w, S, h3, l3);
    bh = stn_pack4(h0, h1, h2, h3); bl = stn_pack4(l0, l1, l2, l3);
  }

  f32x4 acc0[ORS_NT], acc1[ORS_NT];
#pragma unroll
  for (int j = 0; j < ORS_NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc0[j][i] = 0.f; acc1[j][i] = 0.f; }

  const int frag = ors_frag(r, q);
  constexpr int TOPWAIT = STREAM ? 2 : 0;           // memory operations a wave issues per piece behind W's

  // ---- the stream of pieces: 18 tiles of 3 MFMAs out of slot `cur`; in their shadow W's next piece is sent to the other
  // slot (every wave is past this piece's barrier, so nobody reads that slot any more), the piece of A four ahead is sent
  // for (into the ring slot whose piece became planes while the piece before ran) and the next piece becomes planes.
  // Behind the last piece of a block "next" is piece 0 of the workgroup's next block, with an exponent of its own. -----------
  int cur = 0, g = 0;                               // g: pieces so far, the ring position
  for (;;) {
    int Snext = ORS_UNSET;
    for (int s = 0; s < np; ++s, ++g) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TOPWAIT) : "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      const char* fb = smem + cur + frag;
      const bool last = s + 1 == np;
      f16x8 wh[2], wl[2];
      u32x4 nh = __builtin_bit_cast(u32x4, bh), nl = __builtin_bit_cast(u32x4, bl);
      float4 rv0 = make_float4(0.f, 0.f, 0.f, 0.f), rv1 = rv0;
      float mx = 0.f, mo = 0.f;
      int Sn = last ? ORS_UNSET : S;
#define ORS_LOADW(X, J)                                                                                  \
  {                                                                                                      \
    wh[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024, 16));              \
    wl[X] = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + (J) * 1024 + ORS_PLANE, 16));  \
  }
      ORS_LOADW(0, 0)
#pragma unroll
      for (int j = 0; j < ORS_NT; ++j) {
        if (j + 1 < ORS_NT) { ORS_LOADW((j + 1) & 1, j + 1) }
        if (j == 0) {
          dma_w(last ? 0 : s + 1, ORS_PIECE - cur);
          if (STREAM) {
            const bool ahead = ors_ahead_next(s, np);
            dma_raw(ahead ? an0 : ac0, ahead ? an1 : ac1, ors_ahead_piece(s, np), g & (ORS_RING - 1));
          }
          if (ABLATE != 1) {
            const int ro = raw_lane + ((g + 1) & (ORS_RING - 1)) * ORS_RAW;
            rv0 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + ro, 16));
            rv1 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(smem + (ro ^ 16), 16));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        acc0[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j & 1], bh, acc0[j], 0, 0, 0);
        acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[j & 1], bh, acc1[j], 0, 0, 0);
        acc1[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[j & 1], bl, acc1[j], 0, 0, 0);
        if (ABLATE != 1) {
          // the next piece: the row's maximum in three steps, each a tile behind the exchange it waits for, ...
          if (j == 1) { mx = ors_max8(rv0, rv1); mo = __shfl_xor(mx, 16, 64); }
          if (j == 2) { mx = fmaxf(mx, mo); mo = __shfl_xor(mx, 32, 64); }
          if (j == 3) { mx = fmaxf(mx, mo); Sn = ors_step_exp(mx, Sn); }
          // ... then a pair of values between a tile's MFMAs
          if (j >= 5 && (j - 5) % 3 == 0 && j <= 14) {
            const int e = (j - 5) / 3;                  // pair e: values 2 e, 2 e + 1 of the lane's eight
            const float4 rv = (e >> 1) ? rv1 : rv0;
            unsigned hp, lp;
            ors_form2((e & 1) ? rv.z : rv.x, (e & 1) ? rv.w : rv.y, Sn, hp, lp);
            if (e == 0) { nh.x = hp; nl.x = lp; } else if (e == 1) { nh.y = hp; nl.y = lp; }
            else if (e == 2) { nh.z = hp; nl.z = lp; } else { nh.w = hp; nl.w = lp; }
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#undef ORS_LOADW
      bh = __builtin_bit_cast(f16x8, nh); bl = __builtin_bit_cast(f16x8, nl);
      cur = ORS_PIECE - cur;
      if (last) {
        Snext = Sn;
      } else {
        // a row whose exponent moved: its sums so far to the new scale (rare: a row that grows along k)
        if (__builtin_amdgcn_ballot_w64(Sn != S) != 0) {
          const float f = ldexpf(1.f, Sn - S);          // 1 in the lanes that did not move; 0 from "not set yet"
#pragma unroll
          for (int j = 0; j < ORS_NT; ++j) { acc0[j] *= f; acc1[j] *= f; }
        }
        S = Sn;
      }
    }

    // ---- the block's rows: the lane's row, columns 16 j + 4 q .. + 3 of tile j -------------------------------------------
    const int64_t row = ors_lane_row(blk, wave, r);
    // The exponents and the bias come out of LDS (col_sh / col_bias), so the only memory operations of the drain are the
    // residual loads and the stores, and no load sits between two stores: a wait for a load would also wait for every store
    // issued before it (both count in vmcnt, in order), which made each of the 18 tiles two or three memory round trips.
    // The residual is requested ORS_DRAIN tiles at a time, one group ahead of the group being stored.
    if constexpr (EPI == 1) {
      // Every lane walks pass A (the sums over the wave's rows need all 64, and a branch per load costs registers); a row
      // >= M reads the last row like ors_a_row, adds zeros to dw and stores nothing.
      const bool valid = row < p.M;
      const int64_t rowc = ors_min_l(row, p.M - 1);
      // (opaque: taken apart, its loop-invariant part 4 q would be added to every base pointer ahead of the stream of pieces
      // and stay in registers through it)
      int64_t ro = rowc * p.ldc + ors_out_col(0, q);
      asm volatile("" : "+v"(ro));
      auto dy_of = [&](int j) __attribute__((always_inline)) {
        const int4 sv = *reinterpret_cast<const int4*>(__builtin_assume_aligned(col_sh + ors_out_col(j, q), 16));
        float4 o;
        o.x = stn_unscale(acc1[j][0], acc0[j][0], S + sv.x);
        o.y = stn_unscale(acc1[j][1], acc0[j][1], S + sv.y);
        o.z = stn_unscale(acc1[j][2], acc0[j][2], S + sv.z);
        o.w = stn_unscale(acc1[j][3], acc0[j][3], S + sv.w);
        return o;
      };
      const float* xs = p.nx + ro;
      // tile j of the lane: columns ors_out_col(j, q) .. + 3, `cj` floats behind tile 0's, which `ro` holds
      auto cj = [&](int j) __attribute__((always_inline)) { return ors_out_col(j, q) - ors_out_col(0, q); };
      auto x_of = [&](int j) __attribute__((always_inline)) { return *reinterpret_cast<const float4*>(xs + cj(j)); };
      float4 rq[2][ORS_NDRAIN];
#pragma unroll
      for (int i = 0; i < ORS_NDRAIN; ++i) rq[0][i] = x_of(i);
      const float rinv = 1.0f / p.nrms[rowc];
      const bool want_dw = p.dwpart != nullptr;
      int dwo = ORS_N + ors_dw_lds(wave, ors_out_col(0, q));
      asm volatile("" : "+v"(dwo));
      float* dwrow = norm_sh + dwo;
      float dot = 0.f;
      // ---- pass A
#pragma unroll
      for (int g = 0; g < ORS_NT / ORS_NDRAIN; ++g) {
        if (g + 1 < ORS_NT / ORS_NDRAIN) {
#pragma unroll
          for (int i = 0; i < ORS_NDRAIN; ++i) rq[(g + 1) & 1][i] = x_of((g + 1) * ORS_NDRAIN + i);
        }
#pragma unroll
        for (int i = 0; i < ORS_NDRAIN; ++i) {
          const int j = g * ORS_NDRAIN + i;
          const float4 dy = dy_of(j);
          const float4 x4 = rq[g & 1][i];
          const float4 w4 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(norm_sh + ors_out_col(j, q), 16));
          float4 z, dz;
          z.x = x4.x * rinv; z.y = x4.y * rinv; z.z = x4.z * rinv; z.w = x4.w * rinv;
          dz.x = dy.x * w4.x; dz.y = dy.y * w4.y; dz.z = dy.z * w4.z; dz.w = dy.w * w4.w;
          // (pinned: left free, the compiler keeps dy and the tile's weights for pass B and forms dz there, twelve registers per
          // tile in place of the accumulators' eight, and the kernel spills)
          asm volatile("" : "+v"(dz.x), "+v"(dz.y), "+v"(dz.z), "+v"(dz.w));
          dot += (z.x * dz.x + z.y * dz.y) + (z.z * dz.z + z.w * dz.w);
          if (want_dw) {
            float4 c;
            c.x = ors_row16_sum(valid ? dy.x * z.x : 0.f);
            c.y = ors_row16_sum(valid ? dy.y * z.y : 0.f);
            c.z = ors_row16_sum(valid ? dy.z * z.z : 0.f);
            c.w = ors_row16_sum(valid ? dy.w * z.w : 0.f);
            if (r == 0) {
              float4* d = reinterpret_cast<float4*>(__builtin_assume_aligned(dwrow + cj(j), 16));
              float4 s = *d;
              s.x += c.x; s.y += c.y; s.z += c.z; s.w += c.w;
              *d = s;
            }
          }
          acc0[j][0] = dz.x; acc0[j][1] = dz.y; acc0[j][2] = dz.z; acc0[j][3] = dz.w;
          acc1[j][0] = z.x; acc1[j][1] = z.y; acc1[j][2] = z.z; acc1[j][3] = z.w;
          __builtin_amdgcn_sched_barrier(0);        // a tile at a time
        }
      }
      dot += __shfl_xor(dot, 16, 64);               // the same bits in the row's four lanes: both sides add the same two
      dot += __shfl_xor(dot, 32, 64);
      dot = dot / (float)ORS_N;
      // ---- pass B: dx out of the accumulators; the held gradient is requested one group ahead of the group being stored
      // (the rule of the residual loop below)
      if (valid) {
        float* out = p.C + ro;
        auto dx_of = [&](int j) __attribute__((always_inline)) {
          float4 o;
          o.x = (acc0[j][0] - acc1[j][0] * dot) * rinv;
          o.y = (acc0[j][1] - acc1[j][1] * dot) * rinv;
          o.z = (acc0[j][2] - acc1[j][2] * dot) * rinv;
          o.w = (acc0[j][3] - acc1[j][3] * dot) * rinv;
          return o;
        };
        if (p.nex) {
          const float* res = p.nex + ro;
#pragma unroll
          for (int i = 0; i < ORS_NDRAIN; ++i) rq[0][i] = *reinterpret_cast<const float4*>(res + cj(i));
#pragma unroll
          for (int g = 0; g < ORS_NT / ORS_NDRAIN; ++g) {
            if (g + 1 < ORS_NT / ORS_NDRAIN) {
#pragma unroll
              for (int i = 0; i < ORS_NDRAIN; ++i) rq[(g + 1) & 1][i] = *reinterpret_cast<const float4*>(res + cj((g + 1) * ORS_NDRAIN + i));
            }
#pragma unroll
            for (int i = 0; i < ORS_NDRAIN; ++i) {
              const int j = g * ORS_NDRAIN + i;
              float4 o = dx_of(j);
              const float4 r4 = rq[g & 1][i];
              o.x += r4.x; o.y += r4.y; o.z += r4.z; o.w += r4.w;
              *reinterpret_cast<float4*>(out + cj(j)) = o;
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < ORS_NT; ++j) *reinterpret_cast<float4*>(out + cj(j)) = dx_of(j);
        }
      }
    } else if ((ABLATE != 3 || p.M < 0) && row < p.M) {
      float* out = p.C + row * p.ldc + 4 * q;
      auto tile_out = [&](int j) __attribute__((always_inline)) {
        const int4 sv = *reinterpret_cast<const int4*>(__builtin_assume_aligned(col_sh + 16 * j + 4 * q, 16));
        const float4 b4 = *reinterpret_cast<const float4*>(__builtin_assume_aligned(col_bias + 16 * j + 4 * q, 16));
        float4 o;
        o.x = stn_unscale(acc1[j][0], acc0[j][0], S + sv.x) + b4.x;
        o.y = stn_unscale(acc1[j][1], acc0[j][1], S + sv.y) + b4.y;
        o.z = stn_unscale(acc1[j][2], acc0[j][2], S + sv.z) + b4.z;
        o.w = stn_unscale(acc1[j][3], acc0[j][3], S + sv.w) + b4.w;
        return o;
      };
      if (p.residual) {
        const float* res = p.residual + row * p.ldc + 4 * q;
        float4 rq[2][ORS_DRAIN];
#pragma unroll
        for (int i = 0; i < ORS_DRAIN; ++i) rq[0][i] = *reinterpret_cast<const float4*>(res + 16 * i);
#pragma unroll
        for (int g = 0; g < ORS_NT / ORS_DRAIN; ++g) {
          if (g + 1 < ORS_NT / ORS_DRAIN) {
#pragma unroll
            for (int i = 0; i < ORS_DRAIN; ++i) rq[(g + 1) & 1][i] = *reinterpret_cast<const float4*>(res + 16 * ((g + 1) * ORS_DRAIN + i));
          }
#pragma unroll
          for (int i = 0; i < ORS_DRAIN; ++i) {
            const int j = g * ORS_DRAIN + i;
            float4 o = tile_out(j);
            const float4 r4 = rq[g & 1][i];
            o.x += r4.x; o.y += r4.y; o.z += r4.z; o.w += r4.w;
            *reinterpret_cast<float4*>(out + 16 * j) = o;
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < ORS_NT; ++j) *reinterpret_cast<float4*>(out + 16 * j) = tile_out(j);
      }
    }
    // the stores are memory operations like the fetches: the count starts afresh (and behind the last block the repeated
    // fetches must not outlive the workgroup's LDS)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (nxt == blk) break;
    blk = nxt;
    nxt = ors_next_block(blk, grid, nblk);
    ac0 = an0; ac1 = an1;
    an0 = a_src(nxt, 0); an1 = a_src(nxt, 1);
    S = ABLATE == 1 ? 0 : Snext;
#pragma unroll
    for (int j = 0; j < ORS_NT; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) { acc0[j][i] = 0.f; acc1[j][i] = 0.f; }
  }
  // EPI 1: the eight waves' weight-gradient sums, added in a fixed order, are this workgroup's partial row
  if constexpr (EPI == 1) {
    if (p.dwpart) {
      __syncthreads();
      if (tid < ORS_N) {
        const float* s = norm_sh + ORS_N + tid;
        p.dwpart[(int64_t)blockIdx.x * ORS_N + tid] =
            ((s[ors_dw_lds(0, 0)] + s[ors_dw_lds(1, 0)]) + (s[ors_dw_lds(2, 0)] + s[ors_dw_lds(3, 0)])) +
            ((s[ors_dw_lds(4, 0)] + s[ors_dw_lds(5, 0)]) + (s[ors_dw_lds(6, 0)] + s[ors_dw_lds(7, 0)]));
      }
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// Scratch from the library's allocator, with the two-stream rule of RtsTemp (csrc/rowtile_split.hip)
namespace {
struct OrsTemp {
  void* p = nullptr;
  hipStream_t st = nullptr;
  int get(int64_t bytes, void* stream) { st = (hipStream_t)stream; return pdn_malloc(&p, bytes); }
  ~OrsTemp() {
    static const bool two_stream = getenv("PDN_TWO_STREAM") && atoi(getenv("PDN_TWO_STREAM")) != 0;
    if (p && two_stream) (void)hipStreamSynchronize(st);
    if (p) pdn_free(p);
  }
};
}

// PDN_OUTRES_SPLIT=0: the fp32 kernel at every size.  Read on EVERY call (a test switches it in process), announced the
// first time it is seen at 0.
int pdn_outres_split_takes(const float* A, const float* B, const float* C, const float* bias, const float* residual, int M,
                           int K, int64_t lda, int64_t ldb, int64_t ldc, int b_trans, int kb, int64_t b_bstride, int splits,
                           void* stream) {
  if (M < ORS_MIN_ROWS || K < ORS_MIN_K || K > ORS_MAX_K || K % ORS_KP != 0 || splits != 1) return 0;
  if ((lda & 3) || (ldc & 3) || (ldb & 3) || (b_bstride & 3) || lda < K || ldc < ORS_N) return 0;
  if (kb > 0 ? (!b_trans || kb % ORS_KP != 0 || K % kb != 0) : ldb < (b_trans ? K : ORS_N)) return 0;
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)bias | (uintptr_t)residual) & 15) return 0;
  const char* e = getenv("PDN_OUTRES_SPLIT");
  if (e && atoi(e) == 0) {
    static bool s_told = false;
    if (!s_told) {
      s_told = true;
      fprintf(stderr, "[pdnhip] WARNING: PDN_OUTRES_SPLIT=0 -- the layer input gradients, the down projection and the 288 x 288 products stay on the fp32 MFMA kernels\n");
    }
    return 0;
  }
  // the W images come from the library's allocator, which a stream that is being captured must not call
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return cs == hipStreamCaptureStatusNone ? 1 : 0;
}

// `norm` (epilogue 1, csrc/normgrad.hip): the RMSNorm backward of the product in the drain; C is then dx
namespace {
struct OrsNorm {
  const float *x, *w, *rms, *ex;
  float* dwpart;                  // ors_grid(M) x 288 floats, or null
};
}
static int ors_launch(const float* A, const float* B, float* C, const float* bias, const float* residual, int M, int K,
                      int64_t lda, int64_t ldb, int64_t ldc, int b_trans, int kb, int64_t b_bstride, void* stream,
                      int count_slot, const OrsNorm* norm) {
  // both read on every call like PDN_OUTRES_SPLIT (tools/outres_split_probe.py alternates them in one process), the
  // ablation announced the first time it is seen
  const char* ea = getenv("PDN_OUTRES_SPLIT_ABLATE");
  const int ablate = ea ? atoi(ea) : 0;
  if (ablate != 0) {
    static bool s_told = false;
    if (!s_told) {
      s_told = true;
      fprintf(stderr, "[pdnhip] WARNING: PDN_OUTRES_SPLIT_ABLATE=%d -- timing ablation active, the results of the split output-resident products are WRONG\n", ablate);
    }
  }
  // PDN_OUTRES_SPLIT_WGS: workgroups of the main kernel (timing experiments; 0 = one per 128-row block, not persistent)
  const char* eg = getenv("PDN_OUTRES_SPLIT_WGS");
  const int env_wgs = eg ? atoi(eg) : -1;
  const int np = K / ORS_KP;
  hipStream_t st = (hipStream_t)stream;
  // the images and exponents: from the set bound to this thread when it holds exactly this weight in this form
  // (csrc/weight_images.hip), else built here into [images: np pieces | per-piece column maxima: np x 288 | 288 exponents]
  const PdnwDesc key = pdnw_key_ors(B, K, ldb, b_trans, kb, b_bstride);
  OrsWParams w = ors_w_params(key);
  OrsTemp tmp;
  if (!pdnw_lookup(key, stream, &w.wimg, &w.wsh)) {
    const int rc = tmp.get((int64_t)np * ORS_PIECE + (int64_t)np * ORS_N * 4 + ORS_N * 4, stream);
    if (rc) return rc;
    w.wimg = static_cast<char*>(tmp.p); w.pmax = reinterpret_cast<float*>(w.wimg + (int64_t)np * ORS_PIECE);
    w.wsh = reinterpret_cast<int*>(w.pmax + (int64_t)np * ORS_N);
    if (b_trans) {
      hipLaunchKernelGGL(ors_w_max_kernel<false>, dim3(np), dim3(256), 0, st, w);
      hipLaunchKernelGGL(ors_w_img_kernel<false>, dim3(np, ORS_IMG_WGS), dim3(256), 0, st, w);
    } else {
      hipLaunchKernelGGL(ors_w_max_kernel<true>, dim3(np), dim3(256), 0, st, w);
      hipLaunchKernelGGL(ors_w_img_kernel<true>, dim3(np, ORS_IMG_WGS), dim3(256), 0, st, w);
    }
  }
  OrsParams p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.wimg = w.wimg; p.wsh = w.wsh; p.bias = bias; p.residual = residual; p.C = C;
  p.M = M; p.np = np; p.nblk = ors_blocks(M); p.lda = lda; p.ldc = ldc;
  int wgs = ors_grid(M);
  if (env_wgs == 0) wgs = p.nblk;
  else if (env_wgs > 0) wgs = ors_min_i(env_wgs, p.nblk);
  const dim3 grid((unsigned)wgs);
  if (norm) {
    // the partial rows of dw are one per workgroup of ors_grid(M): neither the grid switch nor the ablations apply
    p.nx = norm->x; p.nw = norm->w; p.nrms = norm->rms; p.nex = norm->ex; p.dwpart = norm->dwpart;
    hipLaunchKernelGGL((ors_main_kernel<0, 1>), dim3((unsigned)ors_grid(M)), dim3(512), 0, st, p);
  } else if (ablate == 3) hipLaunchKernelGGL(ors_main_kernel<3>, grid, dim3(512), 0, st, p);
  else STN_LAUNCH_ABLATE(ors_main_kernel, ablate, grid, stream, p);
  pdn_count(count_slot);            // 46 behind outres_launch, 47 for the 288 x 288 products of pdn_gemm_f32
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

int pdn_outres_split_launch(const float* A, const float* B, float* C, const float* bias, const float* residual, int M, int K,
                            int64_t lda, int64_t ldb, int64_t ldc, int b_trans, int kb, int64_t b_bstride, void* stream,
                            int count_slot) {
  return ors_launch(A, B, C, bias, residual, M, K, lda, ldb, ldc, b_trans, kb, b_bstride, stream, count_slot, nullptr);
}

int pdn_outres_split_norm_bwd_partial_rows(int M) { return ors_grid(M); }

// dx = rmsnorm_bwd([d_1 | ... | d_nb] [W_1 | ... | W_nb]^T) (+ ex) in one launch of the product; dwpart (nullable) receives
// pdn_outres_split_norm_bwd_partial_rows(M) rows of 288 partial sums of dw.  The caller has asked pdn_outres_split_takes.
int pdn_outres_split_norm_bwd_launch(const float* A, const float* W, int64_t b_bstride, int kb, int nb, const float* x,
                                     const float* w, const float* rms, const float* ex, float* dx, float* dwpart, int M,
                                     int64_t lda, void* stream) {
  const OrsNorm norm = {x, w, rms, ex, dwpart};
  return ors_launch(A, W, dx, nullptr, nullptr, M, kb * nb, lda, kb, ORS_N, 1, kb, b_bstride, stream, PDN_CNT_OUTRES_SPLIT,
                    &norm);
}
