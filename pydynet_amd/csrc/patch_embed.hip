// CLIP's patch embedding and the L2 row normalisation of its contrastive head (gfx950, fp32).
//
//   llm/clip/model.py:17-32    patch_project: a 6-D transposed copy of the image, reshape, GEMM with the
//                              (C p p) x D kernel, reshape                                       (4 nodes + a copy)
//   llm/clip/model.py:129-130  concat([class_emb, x], -2) + position_emb                         (2 nodes)
//   llm/clip/model.py:198-203  x / sqrt(sum(x^2, 1) + 1e-12) for the image and the text features   (5 nodes each)
//
// Forward: out (N, P+1, D); row 1+g of image n = patch(n, g) . kernel^T + pos[1+g], row 0 = cls + pos[0].  ONE launch of
// an fp32-MFMA GEMM (v_mfma_f32_32x32x2_f32) whose A tile is gathered straight from the NCHW image: the contraction index
// k = (c, py, px) in the reference's order, so 4 consecutive k (k % 4 == 0, p % 4 == 0) are 4 contiguous floats of one
// image row -- one dwordx4 load.  The transposed patch matrix is never written.
// Backward: dkernel (D x C p p) (+)= dOut[:, 1:]^T @ patches -- a TN product contracted over the N P patch rows, the
// patch operand gathered from the image again -- written (or accumulated) straight into the kernel's gradient buffer;
// d(cls) = sum_n dOut[n, 0] and d(pos) = sum_n dOut[n] by a small column-sum launch (fixed order, no atomics).
#include "common.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int PE_KT = 32;          // contraction rows per LDS tile
constexpr int PE_THREADS = 256;    // 4 waves, 2 x 2 over the block tile

struct PeGeom {
  int C, H, W, p, gw, P, D, K;
  int64_t M;                       // N * P patch rows
};

// 32 x 32 tiles per wave: TM x TN; a block is 2 x 2 waves -> (64 TM) x (64 TN).  As / Bs are contraction-major
// ([KT][rows + pad]): lane l of an MFMA reads A[row l & 31][k l >> 5] = As[2s + (l >> 5)][row], 32 consecutive floats.
template <int TM, int TN>
__device__ __forceinline__ void pe_mma(const float* As, int lda, const float* Bs, int ldb, floatx16 (&acc)[TM][TN],
                                       int wm, int wn, int lane) {
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s = 0; s < PE_KT / 2; ++s) {
    float a[TM], b[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) a[i] = As[(2 * s + h) * lda + (wm * TM + i) * 32 + r];
#pragma unroll
    for (int j = 0; j < TN; ++j) b[j] = Bs[(2 * s + h) * ldb + (wn * TN + j) * 32 + r];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// element offset of patch row m (image n, grid cell g) at k = 0
__device__ __forceinline__ int64_t pe_row_base(const PeGeom& G, int64_t m) {
  const int64_t n = m / G.P;
  const int g = (int)(m - n * G.P), gy = g / G.gw, gx = g - gy * G.gw;
  return (n * G.C * G.H + (int64_t)gy * G.p) * G.W + (int64_t)gx * G.p;
}
// element offset of contraction index k (k % 4 == 0) inside a patch
__device__ __forceinline__ int64_t pe_k_off(const PeGeom& G, int k) {
  const int pp = G.p * G.p, c = k / pp, rem = k - c * pp, py = rem / G.p, px = rem - py * G.p;
  return ((int64_t)c * G.H + py) * G.W + px;
}

// ---- forward: C (M x D) = patches (M x K) . kernel^T, epilogue + pos, class rows -------------------------------------
template <int TM, int TN>
__global__ __launch_bounds__(PE_THREADS) void pe_fwd_kernel(const float* __restrict__ img, const float* __restrict__ ker,
                                                            const float* __restrict__ cls, const float* __restrict__ pos,
                                                            float* __restrict__ out, PeGeom G) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int LDA = BM + 2, LDB = BN + 2;        // (+2: the transposing scalar stores of a wave hit 64 distinct banks)
  constexpr int GA = BM * (PE_KT / 4) / PE_THREADS, GB = BN * (PE_KT / 4) / PE_THREADS;
  __shared__ float As[PE_KT * LDA], Bs[PE_KT * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int q = tid & 7, rsub = tid >> 3;          // float4 group along k, row within a 32-row pass

  int64_t abase[GA];
  bool aok[GA];
#pragma unroll
  for (int g = 0; g < GA; ++g) {
    const int64_t m = m0 + rsub + 32 * g;
    aok[g] = m < G.M;
    abase[g] = aok[g] ? pe_row_base(G, m) : 0;
  }
  float4 ra[GA], rb[GB];
  auto load = [&](int kt) {
    const int k = kt * PE_KT + 4 * q;
    const bool kok = k < G.K;
    const int64_t koff = kok ? pe_k_off(G, k) : 0;
#pragma unroll
    for (int g = 0; g < GA; ++g)
      ra[g] = (aok[g] && kok) ? *reinterpret_cast<const float4*>(img + abase[g] + koff) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      const int d = n0 + rsub + 32 * g;
      rb[g] = (d < G.D && kok) ? *reinterpret_cast<const float4*>(ker + (int64_t)d * G.K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int g = 0; g < GA; ++g) {
      float* dst = As + (4 * q) * LDA + rsub + 32 * g;
      dst[0] = ra[g].x; dst[LDA] = ra[g].y; dst[2 * LDA] = ra[g].z; dst[3 * LDA] = ra[g].w;
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      float* dst = Bs + (4 * q) * LDB + rsub + 32 * g;
      dst[0] = rb[g].x; dst[LDB] = rb[g].y; dst[2 * LDB] = rb[g].z; dst[3 * LDB] = rb[g].w;
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int nkt = (G.K + PE_KT - 1) / PE_KT;
  load(0);
  for (int kt = 0; kt < nkt; ++kt) {
    store();
    __syncthreads();
    if (kt + 1 < nkt) load(kt + 1);              // next tile's global loads in flight under this tile's MFMAs
    pe_mma<TM, TN>(As, LDA, Bs, LDB, acc, wm, wn, lane);
    __syncthreads();
  }

  // epilogue: C/D map col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5); patch row m -> token row 1 + g
  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int64_t m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (m >= G.M) continue;
      const int64_t n = m / G.P;
      const int g = (int)(m - n * G.P);
      float* orow = out + (n * (G.P + 1) + 1 + g) * G.D;
      const float* prow = pos + (int64_t)(1 + g) * G.D;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int d = n0 + (wn * TN + j) * 32 + r;
        if (d < G.D) orow[d] = acc[i][j][e] + prow[d];
      }
    }
  // class rows of the images whose first patch row lies in this block's rows
  const int64_t nlo = (m0 + G.P - 1) / G.P;
  const int64_t mhi = m0 + BM < G.M ? m0 + BM : G.M;
  for (int64_t n = nlo; n * G.P < mhi; ++n)
    for (int dd = tid; dd < BN; dd += PE_THREADS) {
      const int d = n0 + dd;
      if (d < G.D) out[n * (G.P + 1) * G.D + d] = cls[d] + pos[d];
    }
}

// ---- backward: C (D x K) (+)= dOut[:, 1:]^T (D x M) . patches (M x K) --------------------------------------------------
template <int TM, int TN>
__global__ __launch_bounds__(PE_THREADS) void pe_wgrad_kernel(const float* __restrict__ img, const float* __restrict__ dout,
                                                              float* __restrict__ dker, int accumulate, PeGeom G) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int LDA = BM + 4, LDB = BN + 4;        // (row-major float4 stores: 16 B aligned rows)
  constexpr int CA = BM / 4, CB = BN / 4;          // float4 per contraction row
  constexpr int RA = PE_THREADS / CA, RB = PE_THREADS / CB;   // contraction rows per pass
  constexpr int GA = PE_KT / RA, GB = PE_KT / RB;
  __shared__ __attribute__((aligned(16))) float As[PE_KT * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[PE_KT * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int d0 = blockIdx.y * BM, k0 = blockIdx.x * BN;
  const int ca = tid % CA, rsa = tid / CA, cb = tid % CB, rsb = tid / CB;
  const int da = d0 + 4 * ca, kb = k0 + 4 * cb;
  const bool daok = da < G.D, kbok = kb < G.K;
  const int64_t kboff = kbok ? pe_k_off(G, kb) : 0;

  float4 ra[GA], rb[GB];
  auto load = [&](int64_t mt) {
#pragma unroll
    for (int g = 0; g < GA; ++g) {
      const int64_t m = mt * PE_KT + rsa + RA * g;
      if (m < G.M && daok) {
        const int64_t n = m / G.P;
        const int64_t row = n * (G.P + 1) + 1 + (m - n * G.P);
        ra[g] = *reinterpret_cast<const float4*>(dout + row * G.D + da);
      } else {
        ra[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      const int64_t m = mt * PE_KT + rsb + RB * g;
      rb[g] = (m < G.M && kbok) ? *reinterpret_cast<const float4*>(img + pe_row_base(G, m) + kboff)
                                : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int g = 0; g < GA; ++g) *reinterpret_cast<float4*>(As + (rsa + RA * g) * LDA + 4 * ca) = ra[g];
#pragma unroll
    for (int g = 0; g < GB; ++g) *reinterpret_cast<float4*>(Bs + (rsb + RB * g) * LDB + 4 * cb) = rb[g];
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int64_t nmt = (G.M + PE_KT - 1) / PE_KT;
  load(0);
  for (int64_t mt = 0; mt < nmt; ++mt) {
    store();
    __syncthreads();
    if (mt + 1 < nmt) load(mt + 1);
    pe_mma<TM, TN>(As, LDA, Bs, LDB, acc, wm, wn, lane);
    __syncthreads();
  }

  const int r = lane & 31, h = lane >> 5;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int d = d0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (d >= G.D) continue;
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int k = k0 + (wn * TN + j) * 32 + r;
        if (k < G.K) {
          float* c = dker + (int64_t)d * G.K + k;
          *c = accumulate ? *c + acc[i][j][e] : acc[i][j][e];
        }
      }
    }
}

// d(pos)[t][d] (+)= sum_n dOut[n][t][d]; d(cls)[d] (+)= sum_n dOut[n][0][d].  One thread per (t, d), fixed order over n.
__global__ void pe_colsum_kernel(const float* __restrict__ dout, float* __restrict__ dcls, int acc_cls,
                                 float* __restrict__ dpos, int acc_pos, int N, int T, int D) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)T * D) return;
  float s = 0.f;
  for (int n = 0; n < N; ++n) s += dout[(int64_t)n * T * D + i];
  if (dpos) dpos[i] = acc_pos ? dpos[i] + s : s;
  if (dcls && i < D) dcls[i] = acc_cls ? dcls[i] + s : s;
}

// ---- L2 row normalisation: y = x / n, n = sqrt(sum x^2 + 1e-12); dx = (dy - y (y . dy)) / n.  One wave per row. -------
__global__ void l2norm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ nrm, int64_t rows,
                                  int cols) {
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* xr = x + row * cols;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += xr[c] * xr[c];
  const float n = sqrtf(wave_sum(s) + 1e-12f);
  if (lane == 0) nrm[row] = n;
  float* yr = y + row * cols;
  for (int c = lane; c < cols; c += 64) yr[c] = xr[c] / n;
}

__global__ void l2norm_bwd_kernel(const float* __restrict__ y, const float* __restrict__ nrm, const float* __restrict__ dy,
                                  float* __restrict__ dx, int64_t rows, int cols) {
  const int lane = threadIdx.x & 63;
  const int64_t row = blockIdx.x * (int64_t)(blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float *yr = y + row * cols, *gr = dy + row * cols;
  float s = 0.f;
  for (int c = lane; c < cols; c += 64) s += yr[c] * gr[c];
  const float dot = wave_sum(s), n = nrm[row];
  float* xr = dx + row * cols;
  for (int c = lane; c < cols; c += 64) xr[c] = (gr[c] - yr[c] * dot) / n;
}

bool pe_geom(int N, int C, int H, int W, int p, int D, PeGeom* G) {
  if (N < 1 || C < 1 || p < 4 || p % 4 != 0 || H < p || W < p || H % p != 0 || W % p != 0 || D < 4 || D % 4 != 0)
    return false;
  const int64_t K = (int64_t)C * p * p, P = (int64_t)(H / p) * (W / p);
  if (K > (1ll << 30) || (int64_t)N * C * H * W >= (1ll << 46) || (int64_t)N * (P + 1) * D >= (1ll << 46)) return false;
  G->C = C; G->H = H; G->W = W; G->p = p; G->gw = W / p; G->P = (int)P; G->D = D; G->K = (int)K; G->M = (int64_t)N * P;
  return true;
}

}  // namespace

extern "C" {

/* 1 when pdn_patch_embed_fwd_f32 / _bwd_f32 take this shape (p % 4 == 0, H and W multiples of p, D % 4 == 0) */
int pdn_patch_embed_supported(int N, int C, int H, int W, int p, int D) {
  PeGeom G;
  return pe_geom(N, C, H, W, p, D, &G) ? 1 : 0;
}

int pdn_patch_embed_fwd_f32(const float* img, const float* kernel, const float* cls, const float* pos, float* out, int N,
                            int C, int H, int W, int p, int D, void* stream) {
  PeGeom G;
  if (!pe_geom(N, C, H, W, p, D, &G)) {
    pdn_set_error("pdn_patch_embed_fwd_f32: shape N=%d C=%d H=%d W=%d p=%d D=%d not supported", N, C, H, W, p, D);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG(img && kernel && cls && pos && out, "pdn_patch_embed_fwd_f32: null operand");
  PDN_CHECK_ARG((((uintptr_t)img | (uintptr_t)kernel) & 15) == 0, "pdn_patch_embed_fwd_f32: 16B alignment");
  const dim3 grid((unsigned)((G.M + 127) / 128), (unsigned)((G.D + 127) / 128));
  hipLaunchKernelGGL((pe_fwd_kernel<2, 2>), grid, dim3(PE_THREADS), 0, (hipStream_t)stream, img, kernel, cls, pos, out, G);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_PATCH_EMBED_FWD);
  return PDN_OK;
}

int pdn_patch_embed_bwd_f32(const float* img, const float* dout, float* dkernel, int acc_kernel, float* dcls, int acc_cls,
                            float* dpos, int acc_pos, int N, int C, int H, int W, int p, int D, void* stream) {
  PeGeom G;
  if (!pe_geom(N, C, H, W, p, D, &G)) {
    pdn_set_error("pdn_patch_embed_bwd_f32: shape N=%d C=%d H=%d W=%d p=%d D=%d not supported", N, C, H, W, p, D);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG(dout, "pdn_patch_embed_bwd_f32: null dout");
  hipStream_t st = (hipStream_t)stream;
  if (dkernel) {
    PDN_CHECK_ARG(img && (((uintptr_t)img | (uintptr_t)dout) & 15) == 0, "pdn_patch_embed_bwd_f32: null image or 16B alignment");
    // 128 x 128 tiles when they alone fill the 256 CUs, 64 x 64 otherwise (ViT-B/32: 768 x 3072 -> 576 workgroups)
    const int64_t big = ((G.D + 127) / 128) * (((int64_t)G.K + 127) / 128);
    if (big >= 256) {
      const dim3 grid((unsigned)((G.K + 127) / 128), (unsigned)((G.D + 127) / 128));
      hipLaunchKernelGGL((pe_wgrad_kernel<2, 2>), grid, dim3(PE_THREADS), 0, st, img, dout, dkernel, acc_kernel, G);
    } else {
      const dim3 grid((unsigned)((G.K + 63) / 64), (unsigned)((G.D + 63) / 64));
      hipLaunchKernelGGL((pe_wgrad_kernel<1, 1>), grid, dim3(PE_THREADS), 0, st, img, dout, dkernel, acc_kernel, G);
    }
    PDN_LAUNCH_CHECK();
  }
  if (dcls || dpos) {
    const int64_t n = (int64_t)(G.P + 1) * G.D;
    hipLaunchKernelGGL(pe_colsum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dout, dcls, acc_cls, dpos,
                       acc_pos, N, G.P + 1, G.D);
    PDN_LAUNCH_CHECK();
  }
  pdn_count(PDN_CNT_PATCH_EMBED_BWD);
  return PDN_OK;
}

int pdn_l2norm_rows_fwd_f32(const float* x, float* y, float* norm, int64_t rows, int cols, void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(x && y && norm && cols > 0, "pdn_l2norm_rows_fwd_f32: bad operand");
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, norm,
                     rows, cols);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_L2NORM_FWD);
  return PDN_OK;
}

int pdn_l2norm_rows_bwd_f32(const float* y, const float* norm, const float* dy, float* dx, int64_t rows, int cols,
                            void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(y && norm && dy && dx && cols > 0, "pdn_l2norm_rows_bwd_f32: bad operand");
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, norm, dy,
                     dx, rows, cols);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_L2NORM_BWD);
  return PDN_OK;
}

}  // extern "C"
