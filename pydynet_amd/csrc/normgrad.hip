// The RMSNorm backward folded into the layer input gradient (include/pdn_normgrad.h, prefix pdng_):
//
//   d(xn) = [d_1 | ... | d_nb] [W_1 | ... | W_nb]^T          pdn_gemm_outres_blocks_nt_f32, no residual
//   dx, dw = rmsnorm_bwd(x, w, rms, d(xn), dx_residual)        pdn_rmsnorm_bwd_f32, 288 columns
//
// Both block norms of a layer follow directly on such a product, and the pair hands d(xn) (tokens x 288) from one kernel to
// the other through memory.  Where the split-fp16 output-resident kernel takes the product, its drain forms dx and the dw
// partial sums itself (ors_main_kernel<0, 1> of csrc/outres_split.hip) and d(xn) never exists; everywhere else this entry
// runs the pair, so callers have one path.  These extend nn/modules/norm.py:245-248; the reference has no counterpart.
#include "common.h"
#include "gemm_prof.h"
#include "gemm_routes.h"
#include "outres_split_index.h"
#include <atomic>

extern "C" int pdn_rmsnorm_bwd_f32(const float* x, const float* w, const float* rms, const float* dy, const float* dx_residual,
                                   float* dx, float* dw, int accumulate_dw, int64_t rows, int cols, void* workspace,
                                   int64_t workspace_bytes, void* stream);
extern "C" int64_t pdn_rmsnorm_bwd_workspace_bytes(int64_t rows, int cols);
extern "C" int pdn_malloc(void** ptr, int64_t bytes);
extern "C" int pdn_free(void* ptr);

static std::atomic<int64_t> s_fused_launches{0};

static inline int64_t png_round16(int64_t b) { return (b + 15) & ~(int64_t)15; }
static inline int64_t png_dxn_bytes(int M) { return png_round16((int64_t)M * ORS_N * 4); }
// the partial rows of dw: the pair's or the fused kernel's, whichever is larger
static inline int64_t png_part_bytes(int M) {
  const int64_t a = pdn_rmsnorm_bwd_workspace_bytes(M, ORS_N), b = (int64_t)pdn_outres_split_norm_bwd_partial_rows(M) * ORS_N * 4;
  return png_round16(a > b ? a : b);
}

extern "C" int pdng_outres_blocks_nt_rmsnorm_bwd_supported(int M, int kb, int nb) {
  return M >= 1 && kb > 0 && kb % ORS_KP == 0 && nb >= 1 && pdn_gemm_outres_supported(M, ORS_N, kb * nb, kb * nb, kb * nb, ORS_N, 1) ? 1 : 0;
}

static bool png_env_off(const char* name) {
  const char* e = getenv(name);
  return e && atoi(e) == 0;
}
// what can be known of the route without the operands: the split kernel's rows and K, and the two switches
static bool png_fused_expected(int M, int kb, int nb) {
  const int64_t K = (int64_t)kb * nb;
  return M >= ORS_MIN_ROWS && kb > 0 && kb % ORS_KP == 0 && K >= ORS_MIN_K && K <= ORS_MAX_K &&
         !png_env_off("PDN_NORM_BWD_FUSE") && !png_env_off("PDN_OUTRES_SPLIT");
}

// [partial rows of dw | d(xn)]; d(xn) only where the two launches are to be expected from the shape and the switches.
// Where they run all the same (a captured stream, operands off 16 bytes, a switch set after the query) the entry takes
// d(xn) from the library's allocator, which a stream that is being captured must not call: PDN_EWORKSPACE there.
extern "C" int64_t pdng_outres_blocks_nt_rmsnorm_bwd_workspace_bytes(int M, int kb, int nb) {
  if (M < 1) return 0;
  return png_part_bytes(M) + (png_fused_expected(M, kb, nb) ? 0 : png_dxn_bytes(M));
}

// d(xn) outside the workspace; the block goes back to the stream-ordered cache when the entry returns
namespace {
struct PngTemp {                   // (the two-stream rule of OrsTemp, csrc/outres_split.hip)
  void* p = nullptr;
  hipStream_t st = nullptr;
  ~PngTemp() {
    static const bool two_stream = getenv("PDN_TWO_STREAM") && atoi(getenv("PDN_TWO_STREAM")) != 0;
    if (p && two_stream) (void)hipStreamSynchronize(st);
    if (p) pdn_free(p);
  }
};
}

extern "C" int64_t pdng_outres_blocks_nt_rmsnorm_bwd_fused_launches(int reset) {
  return reset ? s_fused_launches.exchange(0) : s_fused_launches.load();
}

// PDN_NORM_BWD_FUSE=0: the two launches at every size.  Read on EVERY call (a probe alternates it in process), announced
// the first time it is seen at 0.
static bool png_fuse_enabled() {
  if (png_env_off("PDN_NORM_BWD_FUSE")) {
    static bool s_told = false;
    if (!s_told) {
      s_told = true;
      fprintf(stderr, "[pdnhip] WARNING: PDN_NORM_BWD_FUSE=0 -- the layer input gradient and the RMSNorm backward behind it run as two launches\n");
    }
    return false;
  }
  return true;
}

extern "C" int pdng_outres_blocks_nt_rmsnorm_bwd_f32(const float* A, const float* W, int64_t b_block_stride, int kb, int nb,
                                                     const float* x, const float* w, const float* rms,
                                                     const float* dx_residual, float* dx, float* dw, int accumulate_dw, int M,
                                                     int64_t lda, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M == 0) return PDN_OK;
  PDN_CHECK_ARG(A && W && x && w && rms && dx, "pdng_outres_blocks_nt_rmsnorm_bwd_f32: null operand");
  if (!pdng_outres_blocks_nt_rmsnorm_bwd_supported(M, kb, nb)) {
    pdn_set_error("pdng_outres_blocks_nt_rmsnorm_bwd_f32: unsupported shape M=%d kb=%d nb=%d", M, kb, nb);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG((((uintptr_t)x | (uintptr_t)w | (uintptr_t)dx_residual | (uintptr_t)dx | (uintptr_t)workspace) & 15) == 0,
                "pdng_outres_blocks_nt_rmsnorm_bwd_f32: 16B alignment");
  if (!workspace || workspace_bytes < png_part_bytes(M)) {     // (room for d(xn) is looked at where it is needed)
    pdn_set_error("pdng_outres_blocks_nt_rmsnorm_bwd_f32: workspace too small");
    return PDN_EWORKSPACE;
  }
  float* part = static_cast<float*>(workspace);
  const int K = kb * nb;
  // the question outres_launch asks for the product alone (dx stands for C: the same stride and alignment), and the fused
  // kernel's own: rms is read by single floats
  const bool fused = png_fuse_enabled() && (((uintptr_t)rms & 3) == 0) &&
                     pdn_outres_split_takes(A, W, dx, nullptr, nullptr, M, K, lda, kb, ORS_N, 1, kb, b_block_stride, 1, stream);
  // the product's bracket of pdn_gemm_outres_blocks_nt_f32 (family 3) on either route; on the fused one the norm's backward
  // is inside the launch it times
  const double flops = 2.0 * M * (double)ORS_N * K;
  if (!fused) {
    PngTemp tmp;
    float* dxn = reinterpret_cast<float*>(static_cast<char*>(workspace) + png_part_bytes(M));
    if (workspace_bytes < png_part_bytes(M) + png_dxn_bytes(M)) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        pdn_set_error("pdng_outres_blocks_nt_rmsnorm_bwd_f32: the two launches in a captured stream need %lld bytes of workspace",
                      (long long)(png_part_bytes(M) + png_dxn_bytes(M)));
        return PDN_EWORKSPACE;
      }
      const int rm = pdn_malloc(&tmp.p, png_dxn_bytes(M));
      if (rm) return rm;
      tmp.st = (hipStream_t)stream;
      dxn = static_cast<float*>(tmp.p);
    }
    int rc;
    {
      GemmProfScope prof(3, flops, 0.0, stream);
      rc = pdn_outres_blocks_nt_launch(A, W, b_block_stride, kb, nb, dxn, M, lda, ORS_N, stream);
    }
    if (rc) return rc;
    return pdn_rmsnorm_bwd_f32(x, w, rms, dxn, dx_residual, dx, dw, accumulate_dw, M, ORS_N, part, png_part_bytes(M), stream);
  }
  int rc;
  {
    GemmProfScope prof(3, flops, 0.0, stream);
    rc = pdn_outres_split_norm_bwd_launch(A, W, b_block_stride, kb, nb, x, w, rms, dx_residual, dx, dw ? part : nullptr, M, lda,
                                          stream);
  }
  if (rc) return rc;
  pdn_count(PDN_CNT_OUTRES);        // slot 14 like outres_launch: "the output-resident product", whichever pipe ran it
  s_fused_launches.fetch_add(1);
  if (dw) return pdn_colsum_partials_launch(part, pdn_outres_split_norm_bwd_partial_rows(M), ORS_N, dw, accumulate_dw, stream);
  return PDN_OK;
}
