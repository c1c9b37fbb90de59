// What the output-resident split-fp16 kernels share below their main loops (csrc/lm_head_dx_split.hip, and the two weight
// gradients of the TN pipeline, csrc/lm_head_dw_split.hip and csrc/outres_tn_split.hip): the vector types, the LDS-DMA, the
// pieces of a tile, and the host entry points of the TN pipeline that csrc/gemm.hip routes to.
#pragma once
#include "common.h"
#include "lm_head_split.h"
#include "split_tn_index.h"

// ---- host entry points (not part of the C ABI) ---------------------------------------------------------------------------
// csrc/split_tn_planes.hip: the three passes over x (column maxima, exponents, plane images) into `extra`
// = [images: rows / 32 pieces | 288 exponents]; returns the exponents.  lse and targets given: 37 KiB images whose tails
// hold the row statistics of the next piece; both null: 36 KiB images.
int* stn_x_planes_launch(const float* x, int64_t ldx, int rows, void* extra, const float* lse, const int64_t* targets, void* stream);
// ... the same 36 KiB images and exponents of xn = x * (1 / rms) * w, which is never written, in one launch: the exponents
// follow from w (rms[t] >= sqrt(mean_d x[t][d]^2) is the caller's contract)
int* stn_xn_planes_launch(const float* x, int64_t ldx, const float* w, const float* rms, int rows, void* extra, void* stream);
// csrc/outres_tn_split.hip: the packed layer weight gradients on split-fp16 MFMA
int pdn_outres_tn_split_enabled();
int pdn_outres_tn_split_supported(int M, int nb_cols, int nbatch, int K);
int64_t pdn_outres_tn_split_extra_bytes(int K);
int pdn_outres_tn_split_ranges(int n_all, int K, int plan);
int pdn_outres_tn_split_launch(const float* X, const float* G, float* C, int n_all, int K, int64_t ldx, int64_t ldg,
                               int nb_cols, int k_per_split, void* extra, void* stream);
// ... with X = the RMSNorm output of (x, norm_w, rms), formed by the plane pass (csrc/normplanes.hip, include/pdn_normplanes.h)
int pdn_outres_tn_split_norm_launch(const float* x, const float* norm_w, const float* rms, const float* G, float* C, int n_all,
                                    int K, int64_t ldx, int64_t ldg, int nb_cols, int k_per_split, void* extra, void* stream);
// ... and the down-projection weight gradient dW_down (M x 288) = h^T g2 on the same kernel with the roles swapped and a
// transposed store (one block; slabs M x 288 row-major)
int pdn_down_dw_split_supported(int M, int N, int K);
int pdn_down_dw_split_ranges(int M, int K);
int pdn_down_dw_split_launch(const float* G2, const float* H, float* C, int M, int K, int64_t ldx, int64_t ldg, int k_per_split,
                             void* extra, void* stream);
// csrc/lm_head_dw_split.hip: the lm_head weight gradient on split-fp16 MFMA, same slabs and column-sum slabs as
// pdn_outres_ce_dw_launch
int pdn_outres_ce_dw_split_enabled();
int pdn_outres_ce_dw_split_supported(int64_t rows, int V, int in_features);
int64_t pdn_outres_ce_dw_split_extra_bytes(int64_t rows);
int pdn_outres_ce_dw_split_launch(const float* x, int64_t ldx, const float* logits, float* C, int V, int64_t rows,
                                  int64_t slab, int k_per_split, const float* lse, const int64_t* targets, float gscale,
                                  const float* gdev, float* colsum, void* extra, void* stream);

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 16 bytes per lane from `g` to LDS address `lds` + 16 lane (`lds` wave-uniform).  Issued from inline assembly and so opaque
// to the compiler on purpose (see the head of csrc/lm_head_dx_split.hip): nothing in a main loop is a load in its eyes, the
// waits are written out there.  (m0 is reserved: the compiler keeps nothing in it, and these kernels have no other
// instruction that reads it.)
__device__ __forceinline__ void split_dma16(const void* g, unsigned lds) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds) : "memory");
}

// the fragments of tile J of both planes of an X image; `fb`: the lane's fragment of tile 0 of plane h
__device__ __forceinline__ void stn_load_frag(const char* fb, int J, f16x8& h, f16x8& l) {
  h = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + J * 1024, 16));
  l = *reinterpret_cast<const f16x8*>(__builtin_assume_aligned(fb + J * 1024 + STN_PLANE, 16));
}
// a tile: xh bh into acc0, xl bh + xh bl into acc1
__device__ __forceinline__ void stn_mfma3(f16x8 xh, f16x8 xl, f16x8 bh, f16x8 bl, f32x4& acc0, f32x4& acc1) {
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bh, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, bh, acc1, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bl, acc1, 0, 0, 0);
}
// the VALU work of a pair of B values, in two halves between the tile's three MFMAs
__device__ __forceinline__ void stn_sched_pair() {
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
  __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
  __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
}
// four pairs of halves as one B operand
__device__ __forceinline__ f16x8 stn_pack4(unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
  const u32x4 v = {w0, w1, w2, w3};
  return __builtin_bit_cast(f16x8, v);
}
// both accumulator sets to zero (a macro: through a function taking the arrays by reference the register allocator names
// two SGPRs of the packed kernel's prologue the other way round)
#define STN_CLEAR(acc0, acc1)                                                \
  _Pragma("unroll") for (int j_ = 0; j_ < STN_NT; ++j_)                      \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { acc0[j_][i_] = 0.f; acc1[j_][i_] = 0.f; }
// the two sums of an element back at fp32: (a0 + a1 / 2048) 2^-e
__device__ __forceinline__ float stn_unscale(float a1, float a0, int e) { return ldexpf(fmaf(a1, 1.f / 2048.f, a0), -e); }

// the timing ablations of a main kernel `K<ABLATE>` (its *_ABLATE switch; the results are WRONG): 1 = the planes of the B
// operand are constants, the raw matrix is never read (MFMA + LDS only); 2 = it is fetched once, before the loop (no HBM
// stream)
#define STN_LAUNCH_ABLATE(K, ablate, grid, stream, p)                                              \
  do {                                                                                             \
    if ((ablate) == 1) hipLaunchKernelGGL(K<1>, grid, dim3(512), 0, (hipStream_t)(stream), p);     \
    else if ((ablate) == 2) hipLaunchKernelGGL(K<2>, grid, dim3(512), 0, (hipStream_t)(stream), p); \
    else hipLaunchKernelGGL(K<0>, grid, dim3(512), 0, (hipStream_t)(stream), p);                   \
  } while (0)
