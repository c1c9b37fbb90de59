// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32), gfx950 only.
//
// Replaces the reference's `x.data @ y.data` and the two products in matmul.grad_fn
// (pydynet/core/tensor.py:657-676) which dispatch to OpenBLAS / cuBLAS through `xp`.
//
//   C[b1,b2] = alpha * A[b1,b2] (MxK) * B[b1,b2] (KxN)  (+ bias[N])  (+ beta * C[b1,b2])
//
// Operands are addressed through element strides so that transposed / head-split views
// (q.transpose(0,2,1,3), W.T, x.T ...) are consumed in place, never copied:
//   A(m,k) = A[m*a_rs + k*a_cs]      B(k,n) = B[k*b_rs + n*b_cs]      C(m,n) = C[m*ldc + n]
//
// Kernel structure (one workgroup = 2 or 4 wave64, one wave per SIMD, 2+ workgroups per CU):
//   * block tile BM x BN x BK, wave tile (WM*32) x (WN*32) of 32x32 MFMA accumulators; BK is
//     32 for tiles up to 128x128 and 16 for the 256-wide ones so that every shape keeps
//     <= 74 KB of LDS (two workgroups per CU) and one barrier per >= 2048 MFMA cycles;
//   * global -> registers -> LDS staging, double-buffered in LDS: the loads for tile t+1 are
//     issued before the MFMAs of tile t, and their LDS writes are slotted into the MIDDLE of
//     that MFMA stream (the matrix pipe keeps executing queued MFMAs while the wave issues
//     ds_write), so staging costs no matrix-pipe time; one barrier per k-tile;
//   * the contraction index inside an MFMA is permuted (half-wave h, step j -> k = 8t+4h+j)
//     so a K-contiguous operand is fetched from LDS with ONE ds_read_b128 per four MFMAs
//     and an M/N-contiguous operand with conflict-free ds_read_b32 -- no transposes anywhere;
//   * interior tiles run a bounds-test-free copy of the main loop;
//   * epilogue: accumulators are parked in LDS one 32-row band at a time and written as
//     16-byte pieces (16 lanes cover 256 B of a row) with alpha / bias / beta*C applied;
//   * XCD-aware tile order: each XCD walks a contiguous run of 8x8 super-tiles so the A and
//     B panels it touches stay in its private 4 MiB L2;
//   * split-K (workspace + deterministic reduce) when the output has too few tiles to
//     fill 256 CUs.
// Besides the tiled kernel this file holds the wave-streaming kernels for weight gradients
// (small output, K = tokens: gemm_tn_stream_*), the skinny kernel for one to four output rows
// (decode: gemm_skinny_kernel) and the host-side selection between them (pdn_gemm_f32).
// f32 MFMA is an exact k-ordered fmaf chain, so results match a scalar fp32 dot product
// in a different summation order only (tolerance documented in tests/).
#include "common.h"
#include <vector>
#include <mutex>
#include <stdlib.h>
#include <stdio.h>
#include <type_traits>

#include "gemm_tiled.h"    // GemmParams, tile loaders, gemm_f32_mfma_kernel, split-K reduce
#include "gemm_stream.h"   // gemm_tn_stream_{,lds_,dma_}kernel, gemm_skinny_kernel
#include "split_tn.h"      // host entry points of the split-fp16 weight gradients (pdn_outres_tn_split_*, pdn_outres_ce_dw_split_*)

#include "gemm_select.h"   // TileCfg / kCfgs, the operand layout and the tiled / streaming selector (host-only)
#include "gemm_prof.h"     // pdn_gemm_prof_begin / end, GemmProfScope
#include "gemm_routes.h"   // what pdn_gemm_f32 routes to in the other GEMM files

// ---- host side ----------------------------------------------------------------------

template <int WMV, int WNV, int WM, int WN, int BK, bool VEC, bool MASKS = false>
static void launch_layout(const GemmParams& p, bool a_kin, bool b_kin, dim3 grid, hipStream_t st) {
  constexpr int NT = WMV * WNV * 64;
  if (a_kin && b_kin)
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<WMV, WNV, WM, WN, BK, true, true, VEC, false, MASKS>), grid, dim3(NT), 0, st, p);
  else if (a_kin && !b_kin)
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<WMV, WNV, WM, WN, BK, true, false, VEC, false, MASKS>), grid, dim3(NT), 0, st, p);
  else if (!a_kin && b_kin)
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<WMV, WNV, WM, WN, BK, false, true, VEC, false, MASKS>), grid, dim3(NT), 0, st, p);
  else if (!MASKS && p.colsum && VEC)   // x^T @ g with the bias gradient (column sums of g) fused in
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<WMV, WNV, WM, WN, BK, false, false, VEC, VEC && !MASKS, false>), grid, dim3(NT), 0, st, p);
  else
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<WMV, WNV, WM, WN, BK, false, false, VEC, false, MASKS>), grid, dim3(NT), 0, st, p);
}

// ---- optional per-launch timing of the dominant kernel (bench.py roofline) ------------
static std::mutex g_prof_mu;
static bool g_prof_on = false;
struct ProfRec { hipEvent_t e0, e1; double flops; int family; double bytes = 0.0; };   // family 0: tiled MFMA kernel, 1: wave-streaming TN kernel, 2: row-resident kernel, 3: output-resident kernel, 4: its weight-gradient (TN) form
static std::vector<ProfRec> g_prof;

// for the fused-epilogue entry points of the other GEMM files: time a launch under a family when profiling is on
// (token = index + 1 of the open record, 0 when profiling is off)
int pdn_gemm_prof_begin(int family, double flops, double bytes, void* stream) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_on) return 0;
  ProfRec rec;
  if (hipEventCreate(&rec.e0) != hipSuccess || hipEventCreate(&rec.e1) != hipSuccess) return 0;
  rec.flops = flops; rec.family = family; rec.bytes = bytes;
  (void)hipEventRecord(rec.e0, (hipStream_t)stream);
  g_prof.push_back(rec);
  return (int)g_prof.size();
}
void pdn_gemm_prof_end(int token, void* stream) {
  if (!token) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (token <= (int)g_prof.size()) (void)hipEventRecord(g_prof[token - 1].e1, (hipStream_t)stream);
}

extern "C" int pdn_gemm_prof_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  return PDN_OK;
}

// The row-resident launches with a fused epilogue (family 5: SwiGLU forward / backward, RoPE -- csrc/gemm_rowres.hip) do
// a bandwidth pass inside a GEMM: they are reported apart, with their algorithmic HBM bytes beside their FLOPs.  Collects
// AND removes their records; records left in place are counted with the row-resident family by the call below.
extern "C" int pdn_gemm_prof_collect_fused(double* ms, double* flops, double* bytes, int64_t* launches) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double tm = 0, tf = 0, tb = 0;
  int64_t n = 0;
  std::vector<ProfRec> keep;
  for (auto& r : g_prof) {
    if (r.family != 5) { keep.push_back(r); continue; }
    PDN_HIP(hipEventSynchronize(r.e1));
    float t = 0.f;
    PDN_HIP(hipEventElapsedTime(&t, r.e0, r.e1));
    tm += t; tf += r.flops; tb += r.bytes; n++;
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  g_prof.swap(keep);
  if (ms) *ms = tm;
  if (flops) *flops = tf;
  if (bytes) *bytes = tb;
  if (launches) *launches = n;
  return PDN_OK;
}

// per kernel family: [0] gemm_f32_mfma_kernel (+ its split-K reduce), [1] gemm_tn_stream_*_kernel,
// [2] gemm_rowres_kernel (csrc/gemm_rowres.hip), [3] gemm_outres_kernel, [4] gemm_outres_tn_kernel (csrc/gemm_outres.hip);
// the three output arrays have FIVE entries each
#define PDN_GEMM_FAMILIES 5
extern "C" int pdn_gemm_prof_collect_families(double* ms5, double* flops5, int64_t* launches5) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  double ms[PDN_GEMM_FAMILIES] = {0}, fl[PDN_GEMM_FAMILIES] = {0};
  int64_t n[PDN_GEMM_FAMILIES] = {0};
  for (auto& r : g_prof) {
    PDN_HIP(hipEventSynchronize(r.e1));
    float t = 0.f;
    PDN_HIP(hipEventElapsedTime(&t, r.e0, r.e1));
    const int f = r.family == 5 ? 2 : (r.family < 0 || r.family >= PDN_GEMM_FAMILIES ? 0 : r.family);
    ms[f] += t; fl[f] += r.flops; n[f]++;
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  for (int f = 0; f < PDN_GEMM_FAMILIES; ++f) {
    if (ms5) ms5[f] = ms[f];
    if (flops5) flops5[f] = fl[f];
    if (launches5) launches5[f] = n[f];
  }
  g_prof.clear();
  return PDN_OK;
}

extern "C" int pdn_gemm_prof_collect(double* total_ms, double* total_flops, int64_t* launches) {
  double ms[PDN_GEMM_FAMILIES], fl[PDN_GEMM_FAMILIES];
  int64_t n[PDN_GEMM_FAMILIES];
  int rc = pdn_gemm_prof_collect_families(ms, fl, n);
  if (rc) return rc;
  double tm = 0, tf = 0;
  int64_t tn = 0;
  for (int f = 0; f < PDN_GEMM_FAMILIES; ++f) { tm += ms[f]; tf += fl[f]; tn += n[f]; }
  if (total_ms) *total_ms = tm;
  if (total_flops) *total_flops = tf;
  if (launches) *launches = tn;
  return PDN_OK;
}

extern "C" int64_t pdn_gemm_f32_workspace_bytes(int M, int N, int K, int nbatch) {
  // Enough for up to 64 splits of one output; pdn_gemm_f32 never uses more than it is given.
  // [64 slabs | the shapes of the split-fp16 packed weight gradients (288 rows, two or more blocks, K >= 32768): x's fp16
  //  plane images and 288 exponents, LAST, at the next multiple of 256 bytes: (K / 32) * 36864 + 1152 bytes, whatever
  //  PDN_OUTRES_TN_SPLIT says; the same region for the down-projection weight gradient: one batch, N == 288, M = 512 .. 1024
  //  a multiple of 16, K >= 32768 a multiple of 32]
  const int64_t base = (int64_t)64 * M * N * (int64_t)nbatch * 4;
  if (!pdn_outres_tn_split_supported(M, N, nbatch, K) && !(nbatch == 1 && pdn_down_dw_split_supported(M, N, K))) return base;
  return ((base + 255) & ~(int64_t)255) + pdn_outres_tn_split_extra_bytes(K);
}

// ---- pdn_gemm_f32 proper: one call record, one function per route ---------------------------------------------------------
// A call of pdn_gemm_f32 / pdn_linear_relu_fwd_f32 / pdn_linear_dx_masked_f32: its arguments (those the kernels read are in
// `p`) and the facts the routes derive from them, once.  `relu_mask` / `grad_mask` (GemmParams) are the one-bit-per-element
// epilogues of pdn_linear_relu_fwd_f32 / pdn_linear_dx_masked_f32: with either (`ext_on`), the product goes to the tiled
// kernel unsplit.
struct GemmCall {
  GemmParams p;              // operands, extents, strides, alpha / beta; the launching route sets splits, k_per_split, tiles
  int nb1, nbatch;
  bool ext_on, mask_colsum;
  GemmLayout lay;            // a_kin, b_kin, vec (gemm_select.h)
  int bt;                    // B as the kernels with a row stride and a transpose flag take it: bt = 1: (N x K) row-major
  int64_t ldb;
  void* workspace;           // as passed
  int64_t workspace_bytes;
  int64_t ws_bytes, ws_floats;   // its capacity: 0 without a workspace
  void* stream;
  hipStream_t st;
  // pdn_gemm_outres_tn_blocks_norm (csrc/normplanes.hip): A^T holds the rows BEFORE an RMSNorm with this weight and these
  // row statistics, and the operand is the norm's output, which exists nowhere.  Only route 7's split-fp16 form takes it.
  const float* norm_w = nullptr;
  const float* norm_rms = nullptr;
};
// what a route returns when the call is not its own: the next route is tried
constexpr int kNotTaken = -0x7fffffff - 1;

static inline bool al16(const void* q) { return gemm_al16((uintptr_t)q); }

// the deterministic sum of `p.splits` slabs in p.ws into C (alpha, bias, residual, beta * C applied); `rvec`: 16-byte
// accesses, which every site decides for its own operands
static int reduce_slabs(const GemmParams& p, int64_t total, int nbatch, int rvec, hipStream_t st) {
  const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3(blocks), dim3(256), 0, st, p, nbatch, rvec);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

// ---- 1: one to four output rows (decode): stream the weight matrix once ----------------------
// (a workgroup walks ALL of K for its 128 columns: right when the weight matrix is wide, wrong for a
//  long-K / narrow-N product such as the input-weight gradient of an RNN with one input feature)
static int route_skinny(const GemmCall& c) {
  const GemmParams& p = c.p;
  if (!(p.M <= 4 && !c.ext_on && c.nbatch == 1 && !p.colsum && p.b_cs == 1 && p.a_cs == 1 && gemm_m4(p.N) && gemm_m4(p.b_rs) &&
        gemm_m4(p.ldc) && al16(p.B) && al16(p.C) && (!p.bias || al16(p.bias)) && (!p.residual || al16(p.residual)) && p.K > 0 &&
        (p.K <= 4096 || (int64_t)p.K <= 4ll * p.N)))
    return kNotTaken;
  const dim3 g((p.N + 127) / 128);
  switch (p.M) {
    case 1: hipLaunchKernelGGL((gemm_skinny_kernel<1>), g, dim3(256), 0, c.st, p); break;
    case 2: hipLaunchKernelGGL((gemm_skinny_kernel<2>), g, dim3(256), 0, c.st, p); break;
    case 3: hipLaunchKernelGGL((gemm_skinny_kernel<3>), g, dim3(256), 0, c.st, p); break;
    default: hipLaunchKernelGGL((gemm_skinny_kernel<4>), g, dim3(256), 0, c.st, p); break;
  }
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

// ---- 2: a handful of output columns (a classifier head): bandwidth kernels (gemm_narrow.hip) ----
static int route_narrow(GemmCall& c) {
  GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K;
  if (!(c.nbatch == 1 && !c.ext_on && N <= 16 && p.alpha == 1.f && !p.residual && !p.colsum && !getenv("PDN_GEMM_NO_NARROW")))
    return kNotTaken;
  if (p.beta == 0.f && pdn_gemm_narrow_nn_ok(M, N, K, p.a_rs, p.a_cs, p.A)) {
    if (getenv("PDN_GEMM_DEBUG")) fprintf(stderr, "pdn_gemm_f32 M=%d N=%d K=%d -> narrow NN\n", M, N, K);
    return pdn_gemm_narrow_nn_launch(p.A, p.a_rs, p.B, p.b_rs, p.b_cs, p.bias, p.C, p.ldc, M, N, K, c.stream);
  }
  int kps = 0;
  const int64_t cap = al16(c.workspace) ? c.ws_floats : 0;
  const int sp = !p.bias ? pdn_gemm_narrow_tn_plan(M, N, K, p.a_rs, p.a_cs, p.b_cs, p.A, cap, &kps) : 0;
  if (sp <= 0) return kNotTaken;
  if (getenv("PDN_GEMM_DEBUG")) fprintf(stderr, "pdn_gemm_f32 M=%d N=%d K=%d -> narrow TN (%d slabs)\n", M, N, K, sp);
  const int rc = pdn_gemm_narrow_tn_launch(p.A, p.a_cs, p.B, p.b_rs, (float*)c.workspace, M, N, K, kps, sp, c.stream);
  if (rc) return rc;
  p.splits = sp;
  return reduce_slabs(p, (int64_t)M * N, 1, (N % 4 == 0) && (p.ldc % 4 == 0) && al16(p.C), c.st);
}

// ---- 3: tall A, output exactly the model width (288), longer contraction: outputs resident in accumulators
// (gemm_outres.hip).  Measured against the tiled kernel at 65536 rows: K 768 +6 %, 864 +17 %, 1536 +20 %,
// 32000 +15 % (91.7 % of the matrix peak); at 32768 rows (4-wave workgroups, one wave per SIMD) K >= 1536 only.
static int route_outres(const GemmCall& c) {
  const GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K;
  if (!(c.nbatch == 1 && !c.ext_on && N == 288 && p.a_cs == 1 && p.alpha == 1.f && p.beta == 0.f && !p.colsum && K >= 768 &&
        al16(p.A) && al16(p.B) && !getenv("PDN_GEMM_NO_OUTRES")))
    return kNotTaken;
  const bool big = (M + 255) / 256 >= 224, mid = (M + 127) / 128 >= 224 && K >= 1536;
  // fewer rows than that: K cut into ranges over grid.y (slabs in the workspace), when K is long enough
  int pl_nw, pl_kps;
  // (the plan may also cut K where unsplit 4-wave workgroups would fill the chip: 8-wave ones over two ranges)
  const bool cut = !big && M >= 8192 && K >= 1536 && pdn_gemm_outres_plan(M, K, &pl_nw, &pl_kps) > 1 &&
                   c.ws_bytes >= pdn_gemm_outres_workspace_bytes(M, K);
  if (!((big || mid || cut) && (c.bt || p.b_cs == 1) && pdn_gemm_outres_supported(M, N, K, p.a_rs, c.ldb, p.ldc, c.bt)))
    return kNotTaken;
  GemmProfScope prof(3, 2.0 * M * (double)N * (double)K, 0.0, c.stream);
  if (getenv("PDN_GEMM_DEBUG"))
    fprintf(stderr, "pdn_gemm_f32 M=%d N=%d K=%d -> output-resident (%s)\n", M, N, K, c.bt ? "NT" : "NN");
  return cut ? pdn_gemm_outres_ws_f32(p.A, p.B, p.C, p.bias, p.residual, M, N, K, p.a_rs, c.ldb, p.ldc, c.bt, c.workspace, c.ws_bytes,
                                      c.stream)
             : pdn_gemm_outres_f32(p.A, p.B, p.C, p.bias, p.residual, M, N, K, p.a_rs, c.ldb, p.ldc, c.bt, c.stream);
}

// ---- 4: tall A against a 288 x 288 weight (the attention output projection ctx Wo + x and its input gradient dz Wo^T), 65536
// rows and more: the same output-resident kernel on split-fp16 MFMA (csrc/outres_split.hip, nine pieces) in place of the
// fp32 tile-piece kernel, for exactly the calls that kernel would take.  At 131072 rows 214 (NN, residual) / 202 us (NT)
// on the fp32 pipe against 140 / 104 us here.  Kept away by PDN_OUTRES_SPLIT=0 (read on every call), pdn_gemm_rowtile_mode 3
// (the in-process A/B switch of the row-resident family), PDN_GEMM_NO_OUTRES / PDN_GEMM_NO_ROWRES, a captured stream, and
// operands that overlap C (a residual that IS C is fine: a lane reads its 16 bytes before it writes them).
static int route_outres_split288(const GemmCall& c) {
  const GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K;
  if (!(c.nbatch == 1 && !c.ext_on && N == 288 && K == 288 && p.a_cs == 1 && p.alpha == 1.f && p.beta == 0.f && !p.colsum &&
        !getenv("PDN_GEMM_NO_OUTRES") && !getenv("PDN_GEMM_NO_ROWRES") && pdn_gemm_rowtile_mode(-1) != 3))
    return kNotTaken;
  auto overlaps_c = [&](const float* q, int64_t floats) {
    return q && q < (const float*)p.C + (int64_t)M * p.ldc && (const float*)p.C < q + floats;
  };
  if (!((c.bt || p.b_cs == 1) && pdn_rowtile_plain_ok(M, N, c.bt) && pdn_gemm_rowres_supported(M, N, K, p.a_rs, c.ldb, p.ldc, c.bt) &&
        !overlaps_c(p.A, (int64_t)M * p.a_rs) && !overlaps_c(p.B, (int64_t)288 * c.ldb) &&
        (p.residual == p.C || !overlaps_c(p.residual, (int64_t)M * p.ldc)) &&
        pdn_outres_split_takes(p.A, p.B, p.C, p.bias, p.residual, M, K, p.a_rs, c.ldb, p.ldc, c.bt, 0, 0, 1, c.stream)))
    return kNotTaken;
  if (getenv("PDN_GEMM_DEBUG"))
    fprintf(stderr, "pdn_gemm_f32 M=%d N=%d K=%d -> output-resident, split fp16 (%s)\n", M, N, K, c.bt ? "NT" : "NN");
  GemmProfScope prof(3, 2.0 * M * (double)N * (double)K, 0.0, c.stream);
  return pdn_outres_split_launch(p.A, p.B, p.C, p.bias, p.residual, M, K, p.a_rs, c.ldb, p.ldc, c.bt, 0, 0, c.stream, PDN_CNT_PROJ288_SPLIT);
}

// ---- 5: tall A, contraction 288, wide-enough output: rows of A resident in registers (gemm_rowres.hip) ----
// measured against the tiled kernel at 65536 rows: N 864 +19 %, 1536 +14 %, 768 (either B orientation)
// +11..14 %, 32000 +4 %; N 288 equal (left to the tiled kernel); with a residual the tiled epilogue wins
// A batch whose members share A and write side by side into one packed buffer (x against Wq | Wk | Wv,
// x against Wg | Wu: core/fused/) is ONE such product with B in equally spaced column blocks.
static int route_rowres(const GemmCall& c) {
  const GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K, nbatch = c.nbatch;
  const bool one_dim = c.nb1 == 1 || p.nb2 == 1;
  const int64_t a_bs = c.nb1 == 1 ? p.a_bs2 : p.a_bs1, b_bs = c.nb1 == 1 ? p.b_bs2 : p.b_bs1, c_bs = c.nb1 == 1 ? p.c_bs2 : p.c_bs1;
  const bool blocks = nbatch > 1 && one_dim && a_bs == 0 && c_bs == N && p.ldc >= (int64_t)nbatch * N && !p.bias &&
                      N % 96 == 0 && (b_bs & 3) == 0;
  const int64_t n_all = (int64_t)N * (blocks ? nbatch : 1);
  // (round 5: the tile-piece kernel also takes what the chunk kernel lost to the tiled one -- outputs narrower than 768
  //  columns, i.e. the 288 x 288 products of the attention output projection, and a residual added in the store)
  const bool tilepiece = nbatch == 1 && K == 288 && n_all >= 96 && n_all % 32 == 0 && M >= 8192 &&
                         pdn_rowtile_plain_ok(M, (int)n_all, c.bt);
  if (!((nbatch == 1 || blocks) && !c.ext_on && K == 288 && p.a_cs == 1 && p.alpha == 1.f && p.beta == 0.f && !p.colsum &&
        (tilepiece || (!p.residual && n_all >= 768)) && n_all < (1 << 30) && M >= 8192 && al16(p.A) && al16(p.B) &&
        (!p.residual || al16(p.residual)) && !getenv("PDN_GEMM_NO_ROWRES")))
    return kNotTaken;
  if (!((c.bt || p.b_cs == 1) && pdn_gemm_rowres_supported(M, N, K, p.a_rs, c.ldb, p.ldc, c.bt))) return kNotTaken;
  GemmProfScope prof(2, 2.0 * M * (double)n_all * (double)K, 0.0, c.stream);
  if (getenv("PDN_GEMM_DEBUG"))
    fprintf(stderr, "pdn_gemm_f32 M=%d N=%lld K=%d -> row-resident (%s, %d block%s)\n", M, (long long)n_all, K,
            c.bt ? "NT" : "NN", blocks ? nbatch : 1, blocks ? "s" : "");
  return blocks ? pdn_gemm_rowres_blocks(p.A, p.B, p.C, M, (int)n_all, K, p.a_rs, c.ldb, p.ldc, c.bt, nbatch, b_bs, c.stream)
                : pdn_gemm_rowres_f32(p.A, p.B, p.C, p.bias, p.residual, M, N, K, p.a_rs, c.ldb, p.ldc, c.bt, c.stream);
}

// ---- 6: weight gradient of a wide layer out of the model width: C (288 x N) = x^T (288 x K) g (K x N), K = tokens --
// (the lm_head: N = 32000).  Output-resident over the 288 rows, g read once straight into MFMA operands
// (gemm_outres_tn_kernel); K split so that the grid fills the chip once, slabs combined (with beta) by the reduce.
static int route_outres_tn(GemmCall& c) {
  GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K;
  if (!(c.nbatch == 1 && !c.ext_on && M == 288 && p.a_rs == 1 && p.a_cs >= 288 && p.b_cs == 1 && p.alpha == 1.f && !p.colsum &&
        !p.bias && !p.residual && N >= 8192 && N % 32 == 0 && K % 32 == 0 && K >= 4096 && gemm_m4(p.a_cs) && gemm_m4(p.b_rs) &&
        al16(p.A) && al16(p.B) && (int64_t)288 * p.ldc < (1ll << 30) && (int64_t)32 * p.b_rs < (1ll << 30) &&
        !getenv("PDN_GEMM_NO_OUTRES")))
    return kNotTaken;
  int nw = 8, kps = K;
  const int splits = pdn_gemm_outres_tn_plan(N, K, &nw, &kps);
  const bool direct = splits == 1 && p.beta == 0.f;
  if (!(direct || (int64_t)splits * M * N <= c.ws_floats)) return kNotTaken;
  GemmProfScope prof(4, 2.0 * M * (double)N * (double)K, 0.0, c.stream);
  if (getenv("PDN_GEMM_DEBUG"))
    fprintf(stderr, "pdn_gemm_f32 M=%d N=%d K=%d -> output-resident TN (splits %d)\n", M, N, K, splits);
  const int rc = direct ? pdn_gemm_outres_tn_launch(p.A, p.B, p.C, N, K, p.a_cs, p.b_rs, p.ldc, 0, nw, kps, c.stream)
                        : pdn_gemm_outres_tn_launch(p.A, p.B, (float*)c.workspace, N, K, p.a_cs, p.b_rs, N, (int64_t)M * N, nw, kps,
                                                    c.stream);
  if (rc || direct) return rc;
  p.splits = splits;
  return reduce_slabs(p, (int64_t)M * N, 1, (p.ldc % 4 == 0) && al16(p.C) && al16(c.workspace), c.st);
}

// ---- 7: the packed weight gradients of a transformer block out of the model width: x^T (288 x K) against dq | dk | dv
// (three 288-column blocks of one (K x 864) matrix) or dgate | dup (two 768-column blocks), one output per block.
// The same output-resident TN kernel, K split 40-64 ways so that the grid fills the chip, slabs in the batched
// layout of the split-K reduce (which adds beta * C).  Against the wave-streaming kernel: 864 columns -16 %,
// 1536 columns -11 % (60 instead of 170 operand bytes per MFMA; the slab pass costs 30-40 us).
static int route_outres_tn_blocks(GemmCall& c) {
  GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K, nbatch = c.nbatch;
  const bool one_dim = c.nb1 == 1 || p.nb2 == 1;
  const int64_t a_bs = c.nb1 == 1 ? p.a_bs2 : p.a_bs1, b_bs = c.nb1 == 1 ? p.b_bs2 : p.b_bs1;
  const int64_t n_all = (int64_t)N * nbatch;
  if (!(nbatch > 1 && one_dim && M == 288 && a_bs == 0 && b_bs == N && p.a_rs == 1 && p.a_cs >= 288 && p.b_cs == 1 &&
        p.b_rs >= n_all && p.alpha == 1.f && !p.colsum && !p.bias && !p.residual && N % 32 == 0 && n_all >= 768 && n_all <= 8192 &&
        K % 32 == 0 && K >= 16384 && gemm_m4(p.a_cs) && gemm_m4(p.b_rs) && al16(p.A) && al16(p.B) && !getenv("PDN_GEMM_NO_OUTRES")))
    return kNotTaken;
  int nw = 8, kps = K;
  int splits = pdn_gemm_outres_tn_plan((int)n_all, K, &nw, &kps);
  // split-fp16 form (csrc/outres_tn_split.hip): switched on, a shape it takes, 16-byte aligned operands, and a workspace
  // that holds its extra region behind the 64 slabs (a caller that passes only the slabs selects the fp32 kernel: the
  // in-process A/B switch).  It cuts K into its own number of ranges, at most 64.
  const int64_t xoff = (((int64_t)64 * M * n_all * 4 + 255) & ~(int64_t)255);
  const bool split16 = pdn_outres_tn_split_supported(M, N, nbatch, K) && pdn_outres_tn_split_enabled() && c.workspace &&
                       c.workspace_bytes >= xoff + pdn_outres_tn_split_extra_bytes(K) && al16(c.workspace);
  if (c.norm_w && !split16) return kNotTaken;        // (no fp32 kernel forms the norm: the caller materialises its output)
  if (split16) {
    kps = ((K / 32 + pdn_outres_tn_split_ranges((int)n_all, K, splits) - 1) / pdn_outres_tn_split_ranges((int)n_all, K, splits)) * 32;
    splits = (K + kps - 1) / kps;
  }
  if (!(splits > 1 && (int64_t)splits * M * n_all <= c.ws_floats && nbatch * splits <= 65535)) return kNotTaken;
  GemmProfScope prof(4, 2.0 * M * (double)n_all * (double)K, 0.0, c.stream);
  if (getenv("PDN_GEMM_DEBUG"))
    fprintf(stderr, "pdn_gemm_f32 M=%d N=%lld K=%d -> output-resident TN%s (%d blocks, splits %d)\n", M,
            (long long)n_all, K, split16 ? ", split-fp16" : "", nbatch, splits);
  const int rc = c.norm_w ? pdn_outres_tn_split_norm_launch(p.A, c.norm_w, c.norm_rms, p.B, (float*)c.workspace, (int)n_all, K,
                                                            p.a_cs, p.b_rs, N, kps, (char*)c.workspace + xoff, c.stream)
                 : split16 ? pdn_outres_tn_split_launch(p.A, p.B, (float*)c.workspace, (int)n_all, K, p.a_cs, p.b_rs, N, kps,
                                                      (char*)c.workspace + xoff, c.stream)
                         : pdn_gemm_outres_tn_blocks_launch(p.A, p.B, (float*)c.workspace, (int)n_all, K, p.a_cs, p.b_rs, N, nw, kps,
                                                            c.stream);
  if (rc) return rc;
  p.splits = splits;
  return reduce_slabs(p, (int64_t)M * n_all, nbatch,
                      (p.ldc % 4 == 0) && al16(p.C) && gemm_m4(p.c_bs1) && gemm_m4(p.c_bs2) && al16(c.workspace), c.st);
}

// ---- 8: the down-projection weight gradient dW_down (M x 288) = h^T (M x K) g2 (K x 288), M = 512 .. 1024 in whole waves,
// from 32768 tokens on: the split-fp16 TN kernel with the roles swapped (g2 the plane-image operand, h the raw one) and a
// transposed store (csrc/outres_tn_split.hip), its slabs combined (with beta) by the reduce.  Taken when switched on
// (PDN_OUTRES_TN_SPLIT), with 16-byte aligned operands and a workspace that holds the extra region behind the 64 slabs; a
// caller that passes only the slabs gets the wave-streaming fp32 kernel (the in-process A/B switch).
static int route_down_dw_split(GemmCall& c) {
  GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K;
  if (!(c.nbatch == 1 && !c.ext_on && p.a_rs == 1 && p.b_cs == 1 && p.alpha == 1.f && !p.colsum && !p.bias && !p.residual &&
        pdn_down_dw_split_supported(M, N, K) && p.a_cs >= M && p.b_rs >= N && gemm_m4(p.a_cs) && gemm_m4(p.b_rs) && al16(p.A) &&
        al16(p.B) && c.workspace && al16(c.workspace) && pdn_outres_tn_split_enabled() && !getenv("PDN_GEMM_NO_OUTRES")))
    return kNotTaken;
  const int64_t xoff = (((int64_t)64 * M * N * 4 + 255) & ~(int64_t)255);
  const int ranges = pdn_down_dw_split_ranges(M, K);
  const int kps = ((K / 32 + ranges - 1) / ranges) * 32;
  const int splits = (K + kps - 1) / kps;
  if (!(c.workspace_bytes >= xoff + pdn_outres_tn_split_extra_bytes(K) && splits > 1 && splits <= 64)) return kNotTaken;
  if (getenv("PDN_GEMM_DEBUG"))
    fprintf(stderr, "pdn_gemm_f32 M=%d N=%d K=%d -> output-resident TN, split-fp16, transposed (splits %d)\n", M, N, K, splits);
  GemmProfScope prof(4, 2.0 * M * (double)N * (double)K, 0.0, c.stream);
  const int rc = pdn_down_dw_split_launch(p.B, p.A, (float*)c.workspace, M, K, p.b_rs, p.a_cs, kps, (char*)c.workspace + xoff, c.stream);
  if (rc) return rc;
  p.splits = splits;
  return reduce_slabs(p, (int64_t)M * N, 1, (p.ldc % 4 == 0) && al16(p.C), c.st);
}

// ---- 9: everything else: the wave-streaming weight-gradient kernels or the tiled kernel, as gemm_select.h chooses -------
static int route_stream_or_tiled(GemmCall& c) {
  GemmParams& p = c.p;
  const int M = p.M, N = p.N, K = p.K, nbatch = c.nbatch;
  const bool a_kin = c.lay.a_kin, b_kin = c.lay.b_kin, vec = c.lay.vec;
  const GemmChoice ch = gemm_select(M, N, K, nbatch, p.a_rs, p.b_cs, c.lay, c.ext_on, p.colsum != nullptr, c.mask_colsum, c.ws_floats);
  PDN_CHECK_ARG(ch.cfg >= 0, "pdn_gemm_f32: no tile configuration");
  if (getenv("PDN_GEMM_DEBUG")) {
    char line[256];
    gemm_route_line(line, sizeof(line), M, N, K, nbatch, c.lay, ch);
    fputs(line, stderr);
  }
  p.tiles_m = ch.tiles_m; p.tiles_n = ch.tiles_n; p.k_per_split = ch.k_per_split; p.splits = ch.splits;
  PDN_CHECK_ARG((int64_t)nbatch * p.splits <= 65535, "pdn_gemm_f32: batch*splits too large (%d)",
                nbatch * p.splits);
  dim3 grid(p.tiles_m * p.tiles_n, nbatch * p.splits);
  hipStream_t st = c.st;

  GemmProfScope prof(ch.use_stream ? 1 : 0, 2.0 * M * N * (double)K * nbatch, 0.0, c.stream);
  if (ch.use_stream) {
    constexpr int SNW = kStreamWaves;
    const dim3 sgrid(p.tiles_m * p.tiles_n * p.splits, nbatch);
    switch (ch.kind) {
      case kStreamLdsEdge:                                 // 16-byte loads staged through LDS, edge tests
        switch (ch.sshape) {
          case 0: hipLaunchKernelGGL((gemm_tn_stream_lds_kernel<3, 3, SNW, true>), sgrid, dim3(SNW * 64), 0, st, p); break;
          case 1: hipLaunchKernelGGL((gemm_tn_stream_lds_kernel<5, 2, SNW, true>), sgrid, dim3(SNW * 64), 0, st, p); break;
          case 2: hipLaunchKernelGGL((gemm_tn_stream_lds_kernel<2, 5, SNW, true>), sgrid, dim3(SNW * 64), 0, st, p); break;
          case 3: hipLaunchKernelGGL((gemm_tn_stream_lds_kernel<4, 2, SNW, true>), sgrid, dim3(SNW * 64), 0, st, p); break;
          default: hipLaunchKernelGGL((gemm_tn_stream_lds_kernel<2, 4, SNW, true>), sgrid, dim3(SNW * 64), 0, st, p); break;
        }
        break;
      case kStreamDma: hipLaunchKernelGGL((gemm_tn_stream_dma_kernel<3, 3, SNW>), sgrid, dim3(SNW * 64), 0, st, p); break;
      case kStreamLds: hipLaunchKernelGGL((gemm_tn_stream_lds_kernel<3, 3, SNW, false>), sgrid, dim3(SNW * 64), 0, st, p); break;
      // unaligned operands: dword loads, no LDS
      case kStreamDirect: hipLaunchKernelGGL((gemm_tn_stream_kernel<3, 3, SNW, false>), sgrid, dim3(SNW * 64), 0, st, p); break;
      case kStreamDirectEdge: hipLaunchKernelGGL((gemm_tn_stream_kernel<3, 3, SNW, true>), sgrid, dim3(SNW * 64), 0, st, p); break;
    }
  } else if (c.ext_on) {
    if (!vec) launch_layout<2, 2, 1, 1, 32, false, true>(p, a_kin, b_kin, grid, st);
    else switch (ch.cfg) {
      case 0: launch_layout<2, 2, 2, 2, 32, true, true>(p, a_kin, b_kin, grid, st); break;
      case 3: launch_layout<4, 1, 1, 2, 32, true, true>(p, a_kin, b_kin, grid, st); break;
      case 6: launch_layout<2, 2, 4, 2, 16, true, true>(p, a_kin, b_kin, grid, st); break;
      case 7: launch_layout<2, 2, 2, 4, 16, true, true>(p, a_kin, b_kin, grid, st); break;
      case 8: launch_layout<4, 1, 2, 3, 16, true, true>(p, a_kin, b_kin, grid, st); break;
      default: launch_layout<2, 2, 1, 1, 32, true, true>(p, a_kin, b_kin, grid, st); break;
    }
  } else if (vec) {
    switch (ch.cfg) {
      case 0: launch_layout<2, 2, 2, 2, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 1: launch_layout<4, 1, 1, 3, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 2: launch_layout<1, 4, 3, 1, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 3: launch_layout<4, 1, 1, 2, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 4: launch_layout<1, 4, 2, 1, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 6: launch_layout<2, 2, 4, 2, 16, true>(p, a_kin, b_kin, grid, st); break;
      case 7: launch_layout<2, 2, 2, 4, 16, true>(p, a_kin, b_kin, grid, st); break;
      case 8: launch_layout<4, 1, 2, 3, 16, true>(p, a_kin, b_kin, grid, st); break;
      case 9: launch_layout<1, 4, 3, 2, 16, true>(p, a_kin, b_kin, grid, st); break;
      case 10: launch_layout<2, 1, 1, 3, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 11: launch_layout<1, 2, 3, 1, 32, true>(p, a_kin, b_kin, grid, st); break;
      case 12: launch_layout<4, 1, 1, 3, 16, true>(p, a_kin, b_kin, grid, st); break;
      default: launch_layout<2, 2, 1, 1, 32, true>(p, a_kin, b_kin, grid, st); break;
    }
  } else {
    launch_layout<2, 2, 1, 1, 32, false>(p, a_kin, b_kin, grid, st);
  }
  PDN_LAUNCH_CHECK();
  if (p.splits <= 1) return PDN_OK;
  return reduce_slabs(p, (int64_t)M * N * nbatch, nbatch,
                      (N % 4 == 0) && (p.ldc % 4 == 0) && al16(p.C) && gemm_m4(p.c_bs1) && gemm_m4(p.c_bs2) &&
                          (!p.bias || al16(p.bias)) && (!p.residual || al16(p.residual)) && al16(c.workspace), st);
}

static int gemm_f32_impl(int M, int N, int K, float alpha, const float* A, int64_t a_rs,
                         int64_t a_cs, const float* B, int64_t b_rs, int64_t b_cs, float beta,
                         float* C, int64_t ldc, const float* bias, int nb1, int nb2,
                         int64_t a_bs1, int64_t a_bs2, int64_t b_bs1, int64_t b_bs2,
                         int64_t c_bs1, int64_t c_bs2, const float* residual,
                         float* b_colsum, int colsum_accumulate, void* workspace,
                         int64_t workspace_bytes, void* stream, uint32_t* relu_mask, const uint32_t* grad_mask,
                         float* mask_colsum = nullptr, const float* norm_w = nullptr, const float* norm_rms = nullptr) {
  const bool ext_on = relu_mask || grad_mask;
  PDN_CHECK_ARG(!ext_on || (nb1 == 1 && nb2 == 1 && N % 32 == 0 && !b_colsum),
                "pdn_gemm_f32: the mask epilogues need one batch and N a multiple of 32 (N = %d)", N);
  PDN_CHECK_ARG(M >= 0 && N >= 0 && K >= 0 && nb1 >= 0 && nb2 >= 0, "pdn_gemm_f32: negative extent");
  if (M == 0 || N == 0 || nb1 == 0 || nb2 == 0) return PDN_OK;
  PDN_CHECK_ARG(A && B && C, "pdn_gemm_f32: null operand");
  PDN_CHECK_ARG(ldc >= N, "pdn_gemm_f32: ldc (%lld) < N (%d)", (long long)ldc, N);

  GemmCall c;
  c.norm_w = norm_w; c.norm_rms = norm_rms;
  GemmParams& p = c.p;
  p.A = A; p.B = B; p.C = C; p.bias = bias; p.ws = (float*)workspace;
  p.residual = residual; p.colsum = b_colsum; p.colsum_acc = colsum_accumulate;
  p.relu_mask = relu_mask; p.grad_mask = grad_mask; p.mask_colsum = grad_mask ? mask_colsum : nullptr;
  p.M = M; p.N = N; p.K = K;
  p.a_rs = a_rs; p.a_cs = a_cs; p.b_rs = b_rs; p.b_cs = b_cs; p.ldc = ldc;
  p.nb2 = nb2;
  p.a_bs1 = a_bs1; p.a_bs2 = a_bs2; p.b_bs1 = b_bs1; p.b_bs2 = b_bs2; p.c_bs1 = c_bs1; p.c_bs2 = c_bs2;
  p.alpha = alpha; p.beta = beta;
  c.nb1 = nb1; c.nbatch = nb1 * nb2;
  c.ext_on = ext_on; c.mask_colsum = mask_colsum != nullptr;
  c.lay = gemm_layout(M, N, K, a_rs, a_cs, b_rs, b_cs, a_bs1, a_bs2, b_bs1, b_bs2, (uintptr_t)A, (uintptr_t)B);
  c.bt = (b_rs == 1 && b_cs != 1) ? 1 : 0;
  c.ldb = c.bt ? b_cs : b_rs;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.ws_bytes = (workspace && workspace_bytes > 0) ? workspace_bytes : 0;
  c.ws_floats = c.ws_bytes / 4;
  c.stream = stream; c.st = (hipStream_t)stream;

  if (b_colsum) {
    // fused column sums need B staged n-contiguous, A m-contiguous (the dW = x^T @ g form), the
    // float4 path, a single batch and no k-split (each column is summed by exactly one block)
    if (c.lay.a_kin || c.lay.b_kin || !c.lay.vec || c.nbatch != 1) {
      pdn_set_error("pdn_gemm_f32: b_colsum needs the x^T @ g layout (A m-contiguous, B n-contiguous, aligned, unbatched)");
      return PDN_EUNSUPPORTED;
    }
  }
  // the routes in their order: the first that takes the call launches it
  int rc;
  if (c.norm_w) return route_outres_tn_blocks(c);
  if ((rc = route_skinny(c)) != kNotTaken) return rc;
  if ((rc = route_narrow(c)) != kNotTaken) return rc;
  if ((rc = route_outres(c)) != kNotTaken) return rc;
  if ((rc = route_outres_split288(c)) != kNotTaken) return rc;
  if ((rc = route_rowres(c)) != kNotTaken) return rc;
  if ((rc = route_outres_tn(c)) != kNotTaken) return rc;
  if ((rc = route_outres_tn_blocks(c)) != kNotTaken) return rc;
  if ((rc = route_down_dw_split(c)) != kNotTaken) return rc;
  return route_stream_or_tiled(c);
}

extern "C" int pdn_gemm_f32(int M, int N, int K, float alpha, const float* A, int64_t a_rs,
                            int64_t a_cs, const float* B, int64_t b_rs, int64_t b_cs, float beta,
                            float* C, int64_t ldc, const float* bias, int nb1, int nb2,
                            int64_t a_bs1, int64_t a_bs2, int64_t b_bs1, int64_t b_bs2,
                            int64_t c_bs1, int64_t c_bs2, const float* residual,
                            float* b_colsum, int colsum_accumulate, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  return gemm_f32_impl(M, N, K, alpha, A, a_rs, a_cs, B, b_rs, b_cs, beta, C, ldc, bias, nb1, nb2, a_bs1, a_bs2, b_bs1, b_bs2,
                       c_bs1, c_bs2, residual, b_colsum, colsum_accumulate, workspace, workspace_bytes, stream, nullptr, nullptr);
}

// dW_b (288 x nb_cols, rows ldc apart, blocks c_bs apart) = beta dW_b + xn^T G_b over the nb column blocks of G (K x nb *
// nb_cols, rows ldg apart), xn = x * (1 / rms) * norm_w never written: route 7 alone, with its bracket, counters and slab
// reduce.  PDN_NORMPLANES_NOT_TAKEN where its split-fp16 form does not take the call; the caller then forms xn itself.
int pdn_gemm_outres_tn_blocks_norm(const float* x, const float* norm_w, const float* rms, const float* G, int64_t ldg, float* dW,
                                   int64_t ldc, int64_t c_bs, float beta, int K, int nb_cols, int nb, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  const int rc = gemm_f32_impl(288, nb_cols, K, 1.f, x, 1, 288, G, ldg, 1, beta, dW, ldc, nullptr, 1, nb, 0, 0, 0, nb_cols, 0, c_bs,
                               nullptr, nullptr, 0, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr, norm_w, rms);
  return rc == kNotTaken ? PDN_NORMPLANES_NOT_TAKEN : rc;
}

// ======================================================================================
// `relu(linear(x))` as one product and its backward without an elementwise pass (examples/pydynet/mnist.py:70-78:
// Linear -> ReLU -> Linear -> ReLU -> Linear; nn/functional.py:31-32 relu = maximum(0., x), tensor.py:808-814 its gradient
// passes where out == x, i.e. x >= 0).  The forward stores h = max(0, x W + b) and ONE BIT per element (x W + b >= 0);
// the consumer's input-gradient product applies those bits in its store (pdn_linear_dx_masked_f32), so the gradient
// with respect to the pre-activation is what reaches this layer; anything else uses pdn_relu_mask_bwd_f32.
extern "C" int pdn_relu_mask_supported(int64_t rows, int cols) { return rows > 0 && cols > 0 && cols % 32 == 0; }

extern "C" int pdn_linear_relu_fwd_f32(const float* x, int64_t x_rs, const float* W, int64_t w_rs, int64_t w_cs,
                                       const float* bias, float* h, int64_t ldh, uint32_t* mask, int M, int N, int K,
                                       void* stream) {
  PDN_CHECK_ARG(x && W && h && mask, "pdn_linear_relu_fwd_f32: null operand");
  PDN_CHECK_ARG(pdn_relu_mask_supported(M, N), "pdn_linear_relu_fwd_f32: out features must be a multiple of 32 (N = %d)", N);
  pdn_count(PDN_CNT_LINEAR_RELU_FWD);
  return gemm_f32_impl(M, N, K, 1.f, x, x_rs, 1, W, w_rs, w_cs, 0.f, h, ldh, bias, 1, 1, 0, 0, 0, 0, 0, 0, nullptr, nullptr, 0,
                       nullptr, 0, stream, mask, nullptr);
}

// dx (M x fin) = mask o (g (M x fout) W^T + existing);  W is (fin x fout) with strides (w_rs, w_cs).
// colsum_partials (may be null): (ceil(M / 32) x fin) floats, row b = the column sums of dx over rows 32 b .. 32 b + 31 --
// the bias gradient of the layer below is their sum over b (no pass over dx for it).
extern "C" int pdn_linear_dx_masked_f32(const float* g, int64_t g_rs, const float* W, int64_t w_rs, int64_t w_cs,
                                        float* dx, int64_t ld, const float* existing, const uint32_t* mask,
                                        float* colsum_partials, int M, int fin, int fout, void* stream) {
  PDN_CHECK_ARG(g && W && dx && mask, "pdn_linear_dx_masked_f32: null operand");
  PDN_CHECK_ARG(pdn_relu_mask_supported(M, fin), "pdn_linear_dx_masked_f32: in features must be a multiple of 32 (%d)", fin);
  PDN_CHECK_ARG(!colsum_partials || ((uintptr_t)colsum_partials & 15) == 0, "pdn_linear_dx_masked_f32: unaligned partials");
  pdn_count(PDN_CNT_LINEAR_DX_MASKED);
  return gemm_f32_impl(M, fin, fout, 1.f, g, g_rs, 1, W, w_cs, w_rs, 0.f, dx, ld, nullptr, 1, 1, 0, 0, 0, 0, 0, 0, existing,
                       nullptr, 0, nullptr, 0, stream, nullptr, mask, colsum_partials);
}

__global__ __launch_bounds__(256) void relu_mask_bwd_kernel(const float4* __restrict__ g, const uint32_t* __restrict__ mask,
                                                            float4* __restrict__ dz, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const uint32_t w = mask[i >> 3] >> (4 * (i & 7));
    float4 v = g[i];
    v.x = (w & 1u) ? v.x : 0.f; v.y = (w & 2u) ? v.y : 0.f; v.z = (w & 4u) ? v.z : 0.f; v.w = (w & 8u) ? v.w : 0.f;
    dz[i] = v;
  }
}

// dz = mask o g over a contiguous (rows x cols) array, cols a multiple of 32 (g == dz allowed)
extern "C" int pdn_relu_mask_bwd_f32(const float* g, const uint32_t* mask, float* dz, int64_t rows, int cols, void* stream) {
  PDN_CHECK_ARG(g && mask && dz, "pdn_relu_mask_bwd_f32: null operand");
  PDN_CHECK_ARG(pdn_relu_mask_supported(rows, cols) && (((uintptr_t)g | (uintptr_t)dz) & 15) == 0,
                "pdn_relu_mask_bwd_f32: cols must be a multiple of 32 and the arrays 16-byte aligned");
  const int64_t n4 = rows * cols / 4;
  const int blocks = (int)std::min<int64_t>((n4 + 255) / 256, 8192);
  hipLaunchKernelGGL(relu_mask_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float4*)g, mask, (float4*)dz, n4);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

// ======================================================================================
// SwiGLU in the stores of the tiled kernel, for the model widths the row-resident kernels (csrc/gemm_rowres.hip,
// contraction 288) do not take -- llm/llama/model.py:56-58 forward, its backward through `dh = dy W_down^T`
// (tensor.py:670).  Forward: [Wg | Wu] is packed once per call with its columns in alternating groups of 32 gate / 32 up
// columns (zero-padded to whole 256-column tiles), so a wave's accumulator block holds a gate group and ITS up group side
// by side; the store writes gate, up (the saved [gate | up] layout) and h = silu(gate) * up.  Backward: the store of
// dy W_down^T reads the saved gate / up and writes d[gate | up]; dh never exists.
__global__ __launch_bounds__(256) void swiglu_pack_weights_kernel(const float* __restrict__ wg, int64_t w_stride, float* __restrict__ out,
                                                                  int K, int F, int Np) {
  const int64_t total = (int64_t)K * (Np / 4);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i / (Np / 4)), c = (int)(i - (int64_t)k * (Np / 4)) * 4;       // packed column c .. c + 3
    const int grp = c >> 6, up = (c >> 5) & 1, col = 32 * grp + (c & 31);             // source column in Wg / Wu
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < F) v = *reinterpret_cast<const float4*>(wg + (up ? w_stride : 0) + (int64_t)k * F + col);
    *reinterpret_cast<float4*>(out + (int64_t)k * Np + c) = v;
  }
}

static int swiglu_packed_cols(int F) { return (2 * F + 255) / 256 * 256; }

extern "C" int pdn_gateup_swiglu_tiled_supported(int M, int F, int K) {
  return M >= 4096 && M % 128 == 0 && F >= 256 && F % 32 == 0 && K >= 64 && K % 4 == 0 && !getenv("PDN_NO_TILED_SWIGLU");
}
extern "C" int64_t pdn_gateup_swiglu_tiled_workspace_bytes(int F, int K) { return (int64_t)K * swiglu_packed_cols(F) * 4; }

static void swiglu_params(GemmParams& p, int M, int N, int K, int BM, int BN, int BK) {
  p.bias = nullptr; p.residual = nullptr; p.colsum = nullptr; p.colsum_acc = 0;
  p.relu_mask = nullptr; p.grad_mask = nullptr; p.mask_colsum = nullptr; p.ws = nullptr;
  p.M = M; p.N = N; p.K = K; p.nb2 = 1;
  p.a_bs1 = p.a_bs2 = p.b_bs1 = p.b_bs2 = p.c_bs1 = p.c_bs2 = 0;
  p.alpha = 1.f; p.beta = 0.f; p.splits = 1;
  p.k_per_split = (K + BK - 1) / BK * BK;
  p.tiles_m = (M + BM - 1) / BM; p.tiles_n = (N + BN - 1) / BN;
}

// gu (M x 2 F) = x [Wg | Wu], h (M x F) = silu(gate) * up;  Wg, Wu (K x F) row-major, w_stride floats apart
extern "C" int pdn_gateup_swiglu_tiled_fwd_f32(const float* x, int64_t ldx, const float* w_gate, int64_t w_stride, float* gu,
                                               float* h, int M, int F, int K, void* workspace, int64_t workspace_bytes,
                                               void* stream) {
  PDN_CHECK_ARG(x && w_gate && gu && h && workspace, "pdn_gateup_swiglu_tiled_fwd_f32: null operand");
  PDN_CHECK_ARG(pdn_gateup_swiglu_tiled_supported(M, F, K) && ldx % 4 == 0 && w_stride % 4 == 0 &&
                    ((((uintptr_t)x | (uintptr_t)w_gate | (uintptr_t)gu | (uintptr_t)h | (uintptr_t)workspace) & 15) == 0),
                "pdn_gateup_swiglu_tiled_fwd_f32: unsupported shape or alignment (M %d, F %d, K %d)", M, F, K);
  const int Np = swiglu_packed_cols(F);
  if (workspace_bytes < (int64_t)K * Np * 4) { pdn_set_error("pdn_gateup_swiglu_tiled_fwd_f32: workspace too small"); return PDN_EWORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* packed = (float*)workspace;
  hipLaunchKernelGGL(swiglu_pack_weights_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)K * (Np / 4) + 255) / 256, 2048)), dim3(256), 0, st,
                     w_gate, w_stride, packed, K, F, Np);
  PDN_LAUNCH_CHECK();
  GemmParams p;
  p.A = x; p.B = packed; p.C = gu; p.a_rs = ldx; p.a_cs = 1; p.b_rs = Np; p.b_cs = 1; p.ldc = 2 * (int64_t)F;
  p.swi_h = h; p.swi_gu = nullptr; p.swi_ldh = F; p.swi_F = F;
  GemmProfScope prof(0, 2.0 * M * 2.0 * F * K, 0.0, stream);
  if (Np >= 2048) {                                            // 128 x 256 tiles
    swiglu_params(p, M, Np, K, 128, 256, 16);
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<2, 2, 2, 4, 16, true, false, true, false, false, 1>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, st, p);
  } else {                                                     // 128 x 128
    swiglu_params(p, M, Np, K, 128, 128, 32);
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<2, 2, 2, 2, 32, true, false, true, false, false, 1>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, st, p);
  }
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_TILED_SWIGLU_FWD);
  return PDN_OK;
}

extern "C" int pdn_swiglu_bwd_tiled_supported(int M, int F, int K) {
  return M >= 4096 && M % 128 == 0 && F >= 256 && F % 4 == 0 && K >= 64 && K % 4 == 0 && !getenv("PDN_NO_TILED_SWIGLU");
}

// dgu (M x 2 F) = d[gate | up] from dh = dy (M x K) W_down^T, W_down (F x K) row-major, and the saved gu (M x 2 F)
extern "C" int pdn_swiglu_bwd_tiled_f32(const float* dy, int64_t ldy, const float* w_down, const float* gu, float* dgu, int M,
                                        int F, int K, void* stream) {
  PDN_CHECK_ARG(dy && w_down && gu && dgu, "pdn_swiglu_bwd_tiled_f32: null operand");
  PDN_CHECK_ARG(pdn_swiglu_bwd_tiled_supported(M, F, K) && ldy % 4 == 0 &&
                    ((((uintptr_t)dy | (uintptr_t)w_down | (uintptr_t)gu | (uintptr_t)dgu) & 15) == 0),
                "pdn_swiglu_bwd_tiled_f32: unsupported shape or alignment (M %d, F %d, K %d)", M, F, K);
  hipStream_t st = (hipStream_t)stream;
  GemmParams p;
  p.A = dy; p.B = w_down; p.C = dgu; p.a_rs = ldy; p.a_cs = 1; p.b_rs = 1; p.b_cs = K; p.ldc = 2 * (int64_t)F;
  p.swi_h = nullptr; p.swi_gu = gu; p.swi_ldh = 0; p.swi_F = F;
  GemmProfScope prof(0, 2.0 * M * (double)F * K, 0.0, stream);
  swiglu_params(p, M, F, K, 128, 128, 32);
  hipLaunchKernelGGL((gemm_f32_mfma_kernel<2, 2, 2, 2, 32, true, true, true, false, false, 2>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0, st, p);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_TILED_SWIGLU_BWD);
  return PDN_OK;
}

// ======================================================================================
// Backward of `linear -> cross entropy` (llm/llama/model.py:179 + nn/functional.py:364-381) without the
// (rows x V) gradient of the logits in memory: both products form it from the saved logits as they consume it,
//   dlogits[t][v] = (exp(logits[t][v] - lse[t]) - [v == targets[t]]) * gscale * (upstream ? upstream[0] : 1)
//   dx (rows x in)  = dlogits W^T (+ dx_residual)          W (in x V) row-major
//   dW (in x V)     = dw_beta * dW + x^T dlogits           x (rows x in), row stride ldx
//   dbias (V)       = db_beta * dbias + column sums of dlogits
// in = 288 (output-resident kernels, csrc/gemm_outres.hip).  The cross-entropy pass then only reads the logits
// (row statistics) instead of reading them and writing a gradient of the same size.
// ======================================================================================
// Input gradient of `linear -> cross entropy` from the logits and their ROW MAXIMA (pdn_linear_rowmax_fwd_f32: `max_parts`
// vectors of `rows` maxima), leaving the rows' log-sum-exp as a by-product:
//   dx[t] = gscale * (sum_v exp(l[t][v] - max[t]) W[:, v] / Z[t] - W[:, target[t]]),  Z[t] = sum_v exp(l[t][v] - max[t]),
//   lse[t] = max[t] + log Z[t].
// Independent of the upstream gradient (a scalar factor the caller applies), so a training step can run it in the FORWARD
// pass: the loss is then sum(lse - l[target]) and no pass over the logits for the statistics exists.  W (in x V)
// row-major, in = 288.  workspace: pdn_linear_ce_dx_deferred_workspace_bytes (few rows: the vocabulary is cut into
// ranges over the grid, whose unnormalised rows and row sums a second kernel adds up).
extern "C" int pdn_linear_ce_dx_deferred_f32(const float* logits, const float* rowmax, int max_parts, const int64_t* targets,
                                             float gscale, const float* W, float* dx, float* lse, int64_t rows, int V,
                                             int in_features, void* workspace, int64_t workspace_bytes, void* stream) {
  if (rows == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && rowmax && targets && W && dx && lse && max_parts >= 1, "pdn_linear_ce_dx_deferred_f32: null operand");
  if (!pdn_linear_ce_dx_deferred_supported(rows, V, in_features)) {
    pdn_set_error("pdn_linear_ce_dx_deferred_f32: unsupported shape rows=%lld V=%d in=%d", (long long)rows, V, in_features);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG(((((uintptr_t)logits | (uintptr_t)W) & 15) == 0), "pdn_linear_ce_dx_deferred_f32: 16-byte alignment required");
  GemmProfScope prof(3, 2.0 * (double)rows * (double)V * (double)in_features, 0.0, stream);
  return pdn_outres_ce_dx_deferred_launch(logits, V, rowmax, max_parts, targets, gscale, W, V, dx, in_features, lse,
                                          (int)rows, V, workspace, workspace_bytes, stream);
}

extern "C" int pdn_linear_ce_supported(int64_t rows, int V, int in_features) {
  return in_features == 288 && V % 32 == 0 && V >= 32 && rows % 32 == 0 && rows >= 32 && rows < (1ll << 31) &&
         (int64_t)288 * V < (1ll << 30);
}

extern "C" int64_t pdn_linear_ce_workspace_bytes(int64_t rows, int V, int in_features) {
  if (!pdn_linear_ce_supported(rows, V, in_features)) return 0;
  int nw, kps;
  const int splits = pdn_gemm_outres_tn_plan(V, (int)rows, &nw, &kps);
  // [weight-gradient slabs | column-sum slabs | input-gradient slabs (K split over the grid when rows are few) |
  //  rows >= 32768, V >= 128: x's fp16 plane images and 288 exponents for the split-fp16 weight gradient, LAST, at the next
  //  multiple of 256 bytes: (rows / 32) * 37888 + 1152 bytes, whatever PDN_LMHEAD_DW_SPLIT says]
  const int64_t base = (int64_t)splits * (in_features + 1) * V * 4 + pdn_gemm_outres_workspace_bytes((int)rows, V);
  if (!pdn_outres_ce_dw_split_supported(rows, V, in_features)) return base;
  return ((base + 255) & ~(int64_t)255) + pdn_outres_ce_dw_split_extra_bytes(rows);
}

extern "C" int pdn_linear_ce_backward_f32(const float* x, int64_t ldx, const float* logits, const float* lse,
                                          const int64_t* targets, float gscale, const float* upstream,
                                          const float* W, float* dx, const float* dx_residual, float* dW,
                                          float dw_beta, float* dbias, float db_beta, int64_t rows, int V,
                                          int in_features, void* workspace, int64_t workspace_bytes, void* stream) {
  if (rows == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(x && logits && lse && targets && W, "pdn_linear_ce_backward_f32: null operand");
  if (!pdn_linear_ce_supported(rows, V, in_features)) {
    pdn_set_error("pdn_linear_ce_backward_f32: unsupported shape rows=%lld V=%d in=%d (in 288, V and rows multiples of 32)",
                  (long long)rows, V, in_features);
    return PDN_EUNSUPPORTED;
  }
  PDN_CHECK_ARG((ldx & 3) == 0 && ldx >= in_features && ((((uintptr_t)x | (uintptr_t)logits | (uintptr_t)W) & 15) == 0),
                "pdn_linear_ce_backward_f32: 16-byte alignment required");
  hipStream_t st = (hipStream_t)stream;
  // the two products count as launches of the output-resident family in the GEMM profile (bench.py roofline)
  const double flops = 2.0 * (double)rows * (double)V * (double)in_features;
  if (dx) {
    GemmProfScope prof(3, flops, 0.0, stream);
    int nw_, kps_;
    const int64_t dw_bytes = (int64_t)pdn_gemm_outres_tn_plan(V, (int)rows, &nw_, &kps_) * (in_features + 1) * V * 4;
    const int64_t dx_bytes = pdn_gemm_outres_workspace_bytes((int)rows, V);
    void* dx_ws = (workspace && workspace_bytes >= dw_bytes + dx_bytes && dx_bytes > 0) ? (char*)workspace + dw_bytes : nullptr;
    int rc = pdn_outres_ce_dx_launch(logits, V, lse, targets, gscale, upstream, W, V, dx, in_features, dx_residual,
                                     (int)rows, V, dx_ws, dx_ws ? dx_bytes : 0, stream);
    if (rc) return rc;
  }
  if (dW || dbias) {
    GemmProfScope prof(4, flops, 0.0, stream);
    int nw, kps;
    const int splits = pdn_gemm_outres_tn_plan(V, (int)rows, &nw, &kps);
    const int64_t need = (int64_t)splits * (in_features + 1) * V * 4;
    PDN_CHECK_ARG(workspace && workspace_bytes >= need, "pdn_linear_ce_backward_f32: workspace too small (%lld < %lld)",
                  (long long)workspace_bytes, (long long)need);
    float* slabs = (float*)workspace;
    float* cs = slabs + (int64_t)splits * in_features * V;
    // split-fp16 form: switched on, a shape it takes, and a workspace that holds its extra region behind everything else
    // (a caller that passes only the fp32 kernel's need selects the fp32 kernel: the in-process A/B switch)
    const int64_t xoff = ((need + pdn_gemm_outres_workspace_bytes((int)rows, V) + 255) & ~(int64_t)255);
    const bool split = pdn_outres_ce_dw_split_enabled() && pdn_outres_ce_dw_split_supported(rows, V, in_features) &&
                       workspace_bytes >= xoff + pdn_outres_ce_dw_split_extra_bytes(rows) && (((uintptr_t)workspace & 15) == 0);
    int rc = split ? pdn_outres_ce_dw_split_launch(x, ldx, logits, slabs, V, rows, (int64_t)in_features * V, kps, lse, targets,
                                                   gscale, upstream, dbias ? cs : nullptr, (char*)workspace + xoff, stream)
                   : pdn_outres_ce_dw_launch(x, logits, slabs, V, (int)rows, ldx, V, V, (int64_t)in_features * V, nw, kps, lse,
                                             targets, gscale, upstream, dbias ? cs : nullptr, stream);
    if (rc) return rc;
    GemmParams p{};
    p.N = V; p.nb2 = 1; p.splits = splits;
    if (dW) {
      p.M = in_features; p.C = dW; p.ldc = V; p.ws = slabs; p.beta = dw_beta;
      rc = reduce_slabs(p, (int64_t)p.M * V, 1, al16(dW) && al16(slabs), st);
      if (rc) return rc;
    }
    if (dbias) {
      p.M = 1; p.C = dbias; p.ldc = V; p.ws = cs; p.beta = db_beta;
      rc = reduce_slabs(p, V, 1, al16(dbias) && al16(cs), st);
      if (rc) return rc;
    }
  }
  return PDN_OK;
}
