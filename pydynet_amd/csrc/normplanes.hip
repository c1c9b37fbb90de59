// The weight gradients that contract against an RMSNorm output, from the rows BEFORE the norm (include/pdn_normplanes.h,
// prefix pdnp_):
//
//   dW_b (288 x nb_cols) = beta dW_b + xn^T G_b,     xn[t][d] = x[t][d] * (1 / rms[t]) * w[d],     b = 0 .. nb - 1
//
// the packed products dW_q|k|v = xn1^T dqkv and dW_gate|up = xn2^T dgu of a transformer block (`A^T @ grad` of
// pydynet/core/tensor.py:672-675 behind nn/modules/norm.py:221-248).  Where the split-fp16 TN kernel takes the product
// (csrc/outres_tn_split.hip: route 7 of pdn_gemm_f32, csrc/gemm.hip) its plane pass forms xn on the way into the fp16 planes,
// in one launch instead of three (stn_split_xn_kernel, csrc/split_tn_planes.hip), and xn exists nowhere -- so the forward
// need not write it (pdnp_*_norm_fwd_f32, csrc/gemm_rowres.hip).  Everywhere else this entry writes xn into its workspace
// and runs pdn_gemm_f32 on it, so callers have one path.  The reference has no counterpart.
#include "common.h"
#include "gemm_routes.h"
#include "split_tn.h"
#include <atomic>

extern "C" int pdn_gemm_f32(int M, int N, int K, float alpha, const float* A, int64_t a_rs, int64_t a_cs, const float* B,
                            int64_t b_rs, int64_t b_cs, float beta, float* C, int64_t ldc, const float* bias, int nb1, int nb2,
                            int64_t a_bs1, int64_t a_bs2, int64_t b_bs1, int64_t b_bs2, int64_t c_bs1, int64_t c_bs2,
                            const float* residual, float* b_colsum, int colsum_accumulate, void* workspace,
                            int64_t workspace_bytes, void* stream);
extern "C" int64_t pdn_gemm_f32_workspace_bytes(int M, int N, int K, int nbatch);
extern "C" int pdn_malloc(void** ptr, int64_t bytes);
extern "C" int pdn_free(void* ptr);

static std::atomic<int64_t> s_plane_launches{0};

static inline int64_t pnp_round256(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline int64_t pnp_xn_bytes(int K) { return pnp_round256((int64_t)K * STN_N * 4); }
// the workspace of the product itself, as pydynet_amd/hipnp.py offers it to pdn_gemm_f32 (capped at 256 MiB: the routes take
// what fits)
static inline int64_t pnp_gemm_bytes(int K, int nb_cols, int nb) {
  const int64_t b = pdn_gemm_f32_workspace_bytes(STN_N, nb_cols, K, nb);
  return pnp_round256(b < (1ll << 28) ? b : (1ll << 28));
}

static bool pnp_env_off(const char* name) {
  const char* e = getenv(name);
  return e && atoi(e) == 0;
}
// PDN_NORM_PLANES=0: xn is written and the product runs as before.  Read on EVERY call (a probe and the tests alternate it in
// process), announced the first time it is seen at 0.
static bool pnp_enabled() {
  if (pnp_env_off("PDN_NORM_PLANES")) {
    static bool s_told = false;
    if (!s_told) {
      s_told = true;
      fprintf(stderr, "[pdnhip] WARNING: PDN_NORM_PLANES=0 -- the weight gradients behind an RMSNorm write its output and run the product on it\n");
    }
    return false;
  }
  return true;
}
// what can be known of the route without the operands
static bool pnp_planes_expected(int K, int nb_cols, int nb) {
  return pdn_outres_tn_split_supported(STN_N, nb_cols, nb, K) && nb_cols % 32 == 0 && pdn_outres_tn_split_enabled() &&
         !pnp_env_off("PDN_NORM_PLANES") && !getenv("PDN_GEMM_NO_OUTRES");
}

extern "C" int pdnp_norm_dw_blocks_supported(int K, int nb_cols, int nb) {
  return (K >= 1 && nb >= 1 && nb_cols >= 4 && nb_cols % 4 == 0 && (int64_t)nb_cols * nb < (1 << 24)) ? 1 : 0;
}
// [the product's workspace | xn]; xn only where the plane route is not to be expected from the shape and the switches
extern "C" int64_t pdnp_norm_dw_blocks_workspace_bytes(int K, int nb_cols, int nb) {
  if (!pdnp_norm_dw_blocks_supported(K, nb_cols, nb)) return 0;
  return pnp_gemm_bytes(K, nb_cols, nb) + (pnp_planes_expected(K, nb_cols, nb) ? 0 : pnp_xn_bytes(K));
}
extern "C" int64_t pdnp_norm_dw_blocks_plane_launches(int reset) {
  return reset ? s_plane_launches.exchange(0) : s_plane_launches.load();
}

// xn as the projection kernels leave it: x * (1 / r) * w, one float4 per thread
__global__ __launch_bounds__(256) void pnp_xn_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ rms, float* __restrict__ xn, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / (STN_N / 4);
    const int c4 = (int)(i - row * (STN_N / 4));
    const float inv = 1.f / rms[row];
    const float4 wv = *reinterpret_cast<const float4*>(w + 4 * c4);
    float4 v = *reinterpret_cast<const float4*>(x + 4 * i);
    v.x = v.x * inv * wv.x; v.y = v.y * inv * wv.y; v.z = v.z * inv * wv.z; v.w = v.w * inv * wv.w;
    *reinterpret_cast<float4*>(xn + 4 * i) = v;
  }
}

namespace {
struct PnpTemp {                   // (the two-stream rule of OrsTemp, csrc/outres_split.hip)
  void* p = nullptr;
  hipStream_t st = nullptr;
  ~PnpTemp() {
    static const bool two_stream = getenv("PDN_TWO_STREAM") && atoi(getenv("PDN_TWO_STREAM")) != 0;
    if (p && two_stream) (void)hipStreamSynchronize(st);
    if (p) pdn_free(p);
  }
};
}

extern "C" int pdnp_norm_dw_blocks_f32(const float* x, const float* w, const float* rms, const float* G, int64_t ldg, float* dW,
                                       int64_t dw_block_stride, float beta, int K, int nb_cols, int nb, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  PDN_CHECK_ARG(x && w && rms && G && dW, "pdnp_norm_dw_blocks_f32: null operand");
  if (!pdnp_norm_dw_blocks_supported(K, nb_cols, nb) || ldg < (int64_t)nb_cols * nb) {
    pdn_set_error("pdnp_norm_dw_blocks_f32: unsupported shape K=%d nb_cols=%d nb=%d", K, nb_cols, nb);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)workspace) & 15) == 0 && ((uintptr_t)rms & 3) == 0,
                "pdnp_norm_dw_blocks_f32: 16B alignment");
  const int64_t gbytes = pnp_gemm_bytes(K, nb_cols, nb);
  if (!workspace || workspace_bytes < gbytes) {
    pdn_set_error("pdnp_norm_dw_blocks_f32: workspace too small");
    return PDN_EWORKSPACE;
  }
  if (pnp_enabled()) {
    const int rc = pdn_gemm_outres_tn_blocks_norm(x, w, rms, G, ldg, dW, nb_cols, dw_block_stride, beta, K, nb_cols, nb, workspace,
                                                  gbytes, stream);
    if (rc == PDN_OK) s_plane_launches.fetch_add(1);
    if (rc != PDN_NORMPLANES_NOT_TAKEN) return rc;
  }
  // xn behind the product's workspace, or from the library's allocator (which a stream that is being captured must not call)
  PnpTemp tmp;
  float* xn = reinterpret_cast<float*>(static_cast<char*>(workspace) + gbytes);
  if (workspace_bytes < gbytes + pnp_xn_bytes(K)) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
      (void)hipGetLastError();
      pdn_set_error("pdnp_norm_dw_blocks_f32: the product on a written xn in a captured stream needs %lld bytes of workspace",
                    (long long)(gbytes + pnp_xn_bytes(K)));
      return PDN_EWORKSPACE;
    }
    const int rm = pdn_malloc(&tmp.p, pnp_xn_bytes(K));
    if (rm) return rm;
    tmp.st = (hipStream_t)stream;
    xn = static_cast<float*>(tmp.p);
  }
  const int64_t n4 = (int64_t)K * (STN_N / 4);
  const int blocks = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  hipLaunchKernelGGL(pnp_xn_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, w, rms, xn, n4);
  PDN_LAUNCH_CHECK();
  return pdn_gemm_f32(STN_N, nb_cols, K, 1.f, xn, 1, STN_N, G, ldg, 1, beta, dW, nb_cols, nullptr, 1, nb, 0, 0, 0, nb_cols, 0,
                      dw_block_stride, nullptr, nullptr, 0, workspace, gbytes, stream);
}
