// The device bodies that turn weights into fp16 plane images, compiled into BOTH the per-call passes (rts_w_kernel of
// csrc/rowtile_split.hip, ors_w_max_kernel / ors_w_img_kernel of csrc/outres_split.hip) and the batched builder
// (csrc/weight_images.hip), so that an image is the same bytes whichever built it.  Also the library-internal interface
// of the bound set (pdnw_lookup), which the two launches consult before they run a pass of their own.
#pragma once
#include "common.h"
#include "lm_head_split.h"
#include "weight_images_index.h"

// ---- host: the set bound to this thread (csrc/weight_images.hip) --------------------------------------------------------
// The image (and, for the ors families, the 288 exponents) of the descriptor equal to `key` in the set bound on `stream`;
// false -- and a per-call pass counted -- when there is none, nothing is bound, or PDN_WIMAGES is 0.
bool pdnw_lookup(const PdnwDesc& key, void* stream, char** img, int** wsh);

#if defined(__HIPCC__)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---- rts: one workgroup (256 threads) per tile ------------------------------------------------------------------------
struct RtsWParams {
  const float* B;
  char* wimg;
  int kind, nper;
  int64_t ldb, bstride;
  unsigned g_off, u_off;
};
// the W-params of a descriptor (a product's own key, or a record of a set); the destination is the caller's
inline RtsWParams rts_w_params(const PdnwDesc& d) {
  RtsWParams w;
  memset(&w, 0, sizeof(w));
  w.B = d.B; w.kind = d.kind; w.nper = d.nper; w.ldb = d.ldb; w.bstride = d.bstride; w.g_off = d.g_off; w.u_off = d.u_off;
  return w;
}
#define RTS_W_SM (RTS_K * 33)                // floats of the transposing tile
#define RTS_W_SMAX (8 * 32)
__device__ __forceinline__ void rts_w_tile(const RtsWParams& p, int tile, float* sm, float* smax) {
  const int tid = threadIdx.x, c = tid & 31, kq = tid >> 5;
  float amax = 0.f;
  bool bad = false;
  if (p.kind == 2) {
    // transposed source (the rows of W_down are the tile's columns): read along k, 288 contiguous floats per column
    for (int i = tid; i < 32 * RTS_K; i += 256) {
      const int n = rts_w_t_n(i), k = rts_w_t_k(i);
      sm[k * 33 + n] = p.B[rts_w_src_t(tile, n, k, p.ldb)];
    }
    __syncthreads();
    for (int k = kq; k < RTS_K; k += 8) {
      const float f = sm[k * 33 + c];
      amax = fmaxf(amax, fabsf(f));
      bad |= !(fabsf(f) < INFINITY);
    }
  } else {
    for (int k = kq; k < RTS_K; k += 8) {
      const float f = p.B[rts_w_src(p.kind, tile, c, k, p.nper, p.ldb, p.bstride, p.g_off, p.u_off)];
      sm[k * 33 + c] = f;
      amax = fmaxf(amax, fabsf(f));
      bad |= !(fabsf(f) < INFINITY);
    }
  }
  smax[kq * 32 + c] = bad ? INFINITY : amax;
  __syncthreads();
  char* img = p.wimg + (int64_t)tile * RTS_TILE;
  float cm = smax[c];
#pragma unroll
  for (int i = 1; i < 8; ++i) cm = fmaxf(cm, smax[i * 32 + c]);
  const int sh = ls_shift(cm);                      // (column c: the same for every unit this thread writes)
  for (int u = tid; u < 32 * 36; u += 256) {        // u = 32 ku + n: n == c
    const int ku = u >> 5;
    f16x8 hv, lv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      _Float16 h, l;
      ls_split(sm[(8 * ku + j) * 33 + c], sh, h, l);
      hv[j] = h; lv[j] = l;
    }
    char* dst = img + rts_img_unit(c, ku);
    *reinterpret_cast<f16x8*>(dst) = hv;
    *reinterpret_cast<f16x8*>(dst + RTS_PLANE) = lv;
  }
  if (tid < 32) {
    reinterpret_cast<int*>(img + RTS_TAIL)[tid] = -sh;
    reinterpret_cast<float*>(img + RTS_TAIL + 128)[tid] = 0.f;
  }
}

// ---- ors: the piece images and the column exponents -----------------------------------------------------------------------
struct OrsWParams {
  const float* B;
  float* pmax;                    // np x 288 (the per-call passes only)
  int* wsh;                       // 288 exponents
  char* wimg;                     // np images
  int np, ppb;
  int64_t ldb, bstride;
};
inline OrsWParams ors_w_params(const PdnwDesc& d) {
  OrsWParams w;
  memset(&w, 0, sizeof(w));
  w.B = d.B; w.np = d.n; w.ppb = d.nper; w.ldb = d.ldb; w.bstride = d.bstride;
  return w;
}
#define ORS_W_TILE (ORS_KP * ORS_NN_LD)      // floats of the NN pass's LDS tile

__device__ __forceinline__ float ors_finite_or_inf(float a) { return a < INFINITY ? a : INFINITY; }   // |NaN| -> Inf

// the eight values of unit q of column d of piece `piece`
template <bool NN>
__device__ __forceinline__ void ors_w_unit(const OrsWParams& p, const float* tile, int piece, int d, int q, float (&v)[8]) {
  if (NN) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = tile[ors_nn_lds(8 * q + j, d)];
  } else {
    const float* src = p.B + ors_w_src_nt(piece, d, q, p.ppb, p.ldb, p.bstride);
    const float4 a = *reinterpret_cast<const float4*>(src);
    const float4 b = *reinterpret_cast<const float4*>(src + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}
// NN: float4 c4 .. of the piece's 32 rows of B into the LDS tile (c4_0 = 0, nc4 = 72: whole rows)
__device__ __forceinline__ void ors_w_stage_nn(const OrsWParams& p, float* tile, int piece, int c4_0, int nc4) {
  for (int i = threadIdx.x; i < ORS_KP * nc4; i += 256) {
    const int k = i / nc4, c4 = c4_0 + i % nc4;
    const float4 a = *reinterpret_cast<const float4*>(p.B + ors_w_src_nn(piece, k * 72 + c4, p.ldb));
    float* t = tile + ors_nn_lds(k, 4 * c4);
    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
  }
  __syncthreads();
}
// the largest magnitude of eight values, Inf for a non-finite one
__device__ __forceinline__ float ors_w_max8(const float (&v)[8]) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, ors_finite_or_inf(fabsf(v[j])));
  return m;
}
// unit q of column d of a piece at the column's exponent sh: both planes
__device__ __forceinline__ void ors_w_put(char* img, int d, int q, int sh, const float (&v)[8]) {
  f16x8 hv, lv;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    _Float16 h, l;
    ls_split(v[j], sh, h, l);
    hv[j] = h; lv[j] = l;
  }
  char* dst = img + ors_img_unit(d, q);
  *reinterpret_cast<f16x8*>(dst) = hv;
  *reinterpret_cast<f16x8*>(dst + ORS_PLANE) = lv;
}
#endif
