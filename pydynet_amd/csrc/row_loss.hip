// Cross entropy with reduction='none' (include/pdn_rowloss.h, prefix pdnr_): the row forms of the unfused cross entropy
// (csrc/fused.hip, csrc/masked_loss.hip) and of the lm_head + loss node (csrc/gemm.hip: pdn_linear_ce_backward_f32).  They
// extend nn/functional.py:364-381; the reference has no counterpart.  Statement: pydynet_amd/core/fused/row_loss.py.
//
//   valid[n] = !masked || targets[n] != ignore_index
//   row[n]   = valid[n] ? lse[n] - logits[n][t[n]] : 0
//   dlogits[n] = valid[n] ? (softmax(logits[n]) - onehot(t[n])) * u[n] : 0            u: one upstream number per row
//
// The lm_head products (csrc/gemm_outres.hip, lm_head_dx_split.hip, lm_head_dw_split.hip) take ONE upstream scalar and stay
// as they are.  The per-row factor goes around them: dx rows are scaled after the product; the weight gradient
// x^T diag(u) dz is formed as (diag(u / s) x)^T (s dz) from a scaled copy of x, with s = max |u| as the product's scalar --
// the split-fp16 product keeps one exponent per feature column of x, so rows scaled by u ~ 1 / rows on their own would fall
// into fp16's subnormal range; the bias gradient, a sum the product can only form unweighted, is one pass over the logits.
// Every reduction here has a fixed order; ignored rows are excluded by a select, so u may hold anything there.
#include "common.h"

#define RCE_REG_MAX_V 32768      // 1024 threads x 8 float4 held in registers (MCE_REG_MAX_V of csrc/masked_loss.hip)

extern "C" int pdn_linear_ce_backward_f32(const float* x, int64_t ldx, const float* logits, const float* lse,
                                          const int64_t* targets, float gscale, const float* upstream, const float* W, float* dx,
                                          const float* dx_residual, float* dW, float dw_beta, float* dbias, float db_beta,
                                          int64_t rows, int V, int in_features, void* workspace, int64_t workspace_bytes,
                                          void* stream);

static inline int rce_stream_grid(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
static inline bool rce_reg_row_ok(int V, const void* a, const void* b) {
  return V >= 4096 && V % 4 == 0 && V <= RCE_REG_MAX_V && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
}
static inline int rce_reg_grid(int64_t rows) { return (int)(rows < 256 ? rows : 256); }

// the target of a row as the forward pass read it; valid = false for an ignored row
__device__ __forceinline__ int64_t rce_target(const int64_t* __restrict__ tgt, int64_t row, int masked, int64_t ignore, int V,
                                              bool& valid) {
  int64_t t = tgt[row];
  valid = !masked || t != ignore;
  if (!masked && t < 0) t += V;                      // (the unmasked forward wraps a negative target, csrc/fused.hip)
  return t;
}

// ---- unfused node, generic rows: one workgroup per row, float4 where the row's addresses allow it ---------------------------
__global__ void rce_bwd_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt, int masked, int64_t ignore,
                                    const float* __restrict__ lse_row, const float* __restrict__ u, float* __restrict__ dx,
                                    int64_t rows, int V) {
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * (int64_t)V;
    float* dr = dx + row * (int64_t)V;
    bool valid;
    const int64_t t = rce_target(tgt, row, masked, ignore, V, valid);     // (uniform over the workgroup)
    const float lse = lse_row[row];
    const float g = valid ? u[row] : 0.f;
    const int n4 = ((((uintptr_t)xr | (uintptr_t)dr) & 15) == 0) ? V >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      const int c = 4 * i;
      float4 r;
      r.x = (expf(v.x - lse) - (t == c ? 1.f : 0.f)) * g;
      r.y = (expf(v.y - lse) - (t == c + 1 ? 1.f : 0.f)) * g;
      r.z = (expf(v.z - lse) - (t == c + 2 ? 1.f : 0.f)) * g;
      r.w = (expf(v.w - lse) - (t == c + 3 ? 1.f : 0.f)) * g;
      reinterpret_cast<float4*>(dr)[i] = valid ? r : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int c = n4 * 4 + threadIdx.x; c < V; c += blockDim.x) {
      const float r = (expf(xr[c] - lse) - (c == t ? 1.f : 0.f)) * g;
      dr[c] = valid ? r : 0.f;
    }
  }
}

// ---- unfused node, the row passed through registers (the shapes of mce_reg_kernel of csrc/masked_loss.hip): 4096 <= V <= 32768,
// V % 4 == 0, aligned rows.  The log-sum-exp is saved, so nothing is reduced and no row is read twice: a 1024-thread
// workgroup issues the row's loads (up to 8 float4 per thread in flight), then forms and stores it.  (Holding the next row
// as well, as the kernels with reductions do, does not fit 128 registers without scratch.) -------------------------------------
__global__ __launch_bounds__(1024) void rce_bwd_reg_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                            int masked, int64_t ignore, const float* __restrict__ lse_row,
                                                            const float* __restrict__ u, float* __restrict__ dx, int64_t rows,
                                                            int V) {
  constexpr int NV = RCE_REG_MAX_V / 4 / 1024;     // float4 per thread
  const int n4 = V >> 2, tid = threadIdx.x;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    bool valid;
    const int64_t t = rce_target(tgt, row, masked, ignore, V, valid);
    const float4* xr = reinterpret_cast<const float4*>(x + row * (int64_t)V);
    float4* dr = reinterpret_cast<float4*>(dx + row * (int64_t)V);
    float4 cur[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      cur[j] = i < n4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float lse = lse_row[row];
    const float g = valid ? u[row] : 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      if (i < n4) {
        const int c = 4 * i;
        float4 r;
        r.x = (expf(cur[j].x - lse) - (t == c ? 1.f : 0.f)) * g;
        r.y = (expf(cur[j].y - lse) - (t == c + 1 ? 1.f : 0.f)) * g;
        r.z = (expf(cur[j].z - lse) - (t == c + 2 ? 1.f : 0.f)) * g;
        r.w = (expf(cur[j].w - lse) - (t == c + 3 ? 1.f : 0.f)) * g;
        dr[i] = valid ? r : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
}

// ---- lm_head node: the finish after the projection (mce_finish_rows_kernel of csrc/masked_loss.hip, no reduction) -----------
__global__ void rce_finish_rows_kernel(const float* __restrict__ logits, int64_t ldl, float* __restrict__ lse,
                                       const int64_t* __restrict__ tgt, int masked, int64_t ignore, int64_t rows, int V,
                                       float* __restrict__ loss_row, int64_t* __restrict__ safe, int* __restrict__ err) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= rows) return;
  int64_t t = tgt[r];
  if (masked && t == ignore) {
    loss_row[r] = 0.f;
    safe[r] = V;
    lse[r] = INFINITY;
    return;
  }
  if (t < 0 || t >= V) { *err = 1; t = 0; }
  loss_row[r] = lse[r] - logits[r * ldl + t];
  safe[r] = t;
}

// ---- rows scaled by their upstream number, ignored rows set to 0 ---------------------------------------------------------------
template <bool VEC>
__global__ void rce_scale_rows_kernel(const float* __restrict__ in, int64_t ld_in, float* __restrict__ out, int64_t ld_out,
                                      int64_t rows, int cols, const float* __restrict__ u, const float* __restrict__ inv_s,
                                      const int64_t* __restrict__ safe, int V) {
  const float is = inv_s ? inv_s[0] : 1.f;
  const int per = VEC ? cols >> 2 : cols;
  const int64_t total = rows * per, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / per;
    const int c = (int)(i - r * per);
    const bool keep = safe[r] != V;
    const float f = keep ? u[r] * is : 0.f;
    if (VEC) {
      float4 v = reinterpret_cast<const float4*>(in + r * ld_in)[c];
      v.x *= f; v.y *= f; v.z *= f; v.w *= f;
      reinterpret_cast<float4*>(out + r * ld_out)[c] = keep ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const float v = in[r * ld_in + c] * f;
      out[r * ld_out + c] = keep ? v : 0.f;
    }
  }
}

// ---- largest |u| over the kept rows and its reciprocal: one workgroup ----------------------------------------------------------
__global__ __launch_bounds__(1024) void rce_abs_max_kernel(const float* __restrict__ u, const int64_t* __restrict__ safe, int V,
                                                            int64_t rows, float* __restrict__ s_out) {
  __shared__ float red[16];
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < rows; i += 1024) m = fmaxf(m, safe[i] != V ? fabsf(u[i]) : 0.f);
  m = block_max(m, red);
  if (threadIdx.x == 0) {
    s_out[0] = m;
    s_out[1] = m > 0.f ? 1.f / m : 0.f;
  }
}

// ---- weighted column sums of dlogits: a workgroup owns a row slab x 256 * VEC columns, a thread VEC columns ------------------
template <int VEC>
__global__ __launch_bounds__(256) void rce_colsum_part_kernel(const float* __restrict__ logits, int64_t ldl,
                                                               const float* __restrict__ lse, const int64_t* __restrict__ safe,
                                                               const float* __restrict__ u, int64_t rows, int V,
                                                               int64_t rows_per_slab, float* __restrict__ part) {
  const int c0 = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (c0 >= V) return;                              // (no barrier below)
  const int64_t r0 = blockIdx.y * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  float acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
  int64_t r = r0;
  if (VEC == 4) {
    // four rows in flight; a row's terms enter the sum in row order whatever the batch
    for (; r + 4 <= r1; r += 4) {
      float4 v[4];
      int64_t t[4];
      float l[4], w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = *reinterpret_cast<const float4*>(logits + (r + q) * ldl + c0);
        t[q] = safe[r + q];
        l[q] = lse[r + q];
        w[q] = u[r + q];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool keep = t[q] != V;
        const float a0 = w[q] * (expf(v[q].x - l[q]) - (t[q] == c0 ? 1.f : 0.f));
        const float a1 = w[q] * (expf(v[q].y - l[q]) - (t[q] == c0 + 1 ? 1.f : 0.f));
        const float a2 = w[q] * (expf(v[q].z - l[q]) - (t[q] == c0 + 2 ? 1.f : 0.f));
        const float a3 = w[q] * (expf(v[q].w - l[q]) - (t[q] == c0 + 3 ? 1.f : 0.f));
        acc[0] += keep ? a0 : 0.f;
        acc[1 % VEC] += keep ? a1 : 0.f;
        acc[2 % VEC] += keep ? a2 : 0.f;
        acc[3 % VEC] += keep ? a3 : 0.f;
      }
    }
  }
  for (; r < r1; ++r) {
    const int64_t t = safe[r];
    if (t == V) continue;                           // (uniform over the workgroup)
    const float l = lse[r], w = u[r];
    const float* zr = logits + r * ldl + c0;
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] += w * (expf(zr[k] - l) - (t == c0 + k ? 1.f : 0.f));
  }
  float* p = part + (int64_t)blockIdx.y * V + c0;
#pragma unroll
  for (int k = 0; k < VEC; ++k) p[k] = acc[k];
}
// the slabs' partial rows added up, one thread per column, slabs in their order
__global__ __launch_bounds__(256) void rce_colsum_reduce_kernel(const float* __restrict__ part, int slabs, int V,
                                                                 float* __restrict__ out, float beta) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= V) return;
  float s = 0.f;
  for (int b = 0; b < slabs; ++b) s += part[(int64_t)b * V + c];
  out[c] = beta != 0.f ? beta * out[c] + s : s;
}

// =============================================================================================================================
// slabs of rows for the column sums: about 2048 workgroups over the (column range, slab) grid, at least 64 rows per slab
static void rce_colsum_plan(int64_t rows, int V, int vec, int* slabs, int64_t* rows_per_slab) {
  const int col_tiles = (V + 256 * vec - 1) / (256 * vec);
  int64_t want = 2048 / col_tiles;
  if (want < 1) want = 1;
  const int64_t most = (rows + 63) / 64;
  if (want > most) want = most;
  const int64_t rps = (rows + want - 1) / want;
  *rows_per_slab = rps;
  *slabs = (int)((rows + rps - 1) / rps);
}

extern "C" int64_t pdnr_weighted_colsum_workspace_bytes(int64_t rows, int V) {
  if (rows <= 0 || V <= 0) return 0;
  int s1, s4;
  int64_t rps;
  rce_colsum_plan(rows, V, 1, &s1, &rps);
  rce_colsum_plan(rows, V, 4, &s4, &rps);
  return (int64_t)(s1 > s4 ? s1 : s4) * V * 4;
}

static int rce_colsum(const float* logits, int64_t ldl, const float* lse, const int64_t* safe, const float* u, int64_t rows, int V,
                      float* dbias, float db_beta, void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (!workspace || workspace_bytes < pdnr_weighted_colsum_workspace_bytes(rows, V)) {
    pdn_set_error("pdnr_weighted_colsum_f32: workspace too small");
    return PDN_EWORKSPACE;
  }
  const bool vec = V % 4 == 0 && ldl % 4 == 0 && (((uintptr_t)logits & 15) == 0);
  int slabs;
  int64_t rps;
  rce_colsum_plan(rows, V, vec ? 4 : 1, &slabs, &rps);
  const dim3 g((unsigned)((V + (vec ? 1024 : 256) - 1) / (vec ? 1024 : 256)), (unsigned)slabs);
  if (vec)
    hipLaunchKernelGGL((rce_colsum_part_kernel<4>), g, dim3(256), 0, st, logits, ldl, lse, safe, u, rows, V, rps, (float*)workspace);
  else
    hipLaunchKernelGGL((rce_colsum_part_kernel<1>), g, dim3(256), 0, st, logits, ldl, lse, safe, u, rows, V, rps, (float*)workspace);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(rce_colsum_reduce_kernel, dim3((V + 255) / 256), dim3(256), 0, st, (const float*)workspace, slabs, V, dbias,
                     db_beta);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

static int rce_scale_rows(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows, int cols, const float* u,
                          const float* inv_s, const int64_t* safe, int V, hipStream_t st) {
  const bool vec = cols % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ((((uintptr_t)in | (uintptr_t)out) & 15) == 0);
  const int64_t total = rows * (vec ? cols / 4 : cols);
  if (vec)
    hipLaunchKernelGGL((rce_scale_rows_kernel<true>), dim3(rce_stream_grid(total)), dim3(256), 0, st, in, ld_in, out, ld_out, rows,
                       cols, u, inv_s, safe, V);
  else
    hipLaunchKernelGGL((rce_scale_rows_kernel<false>), dim3(rce_stream_grid(total)), dim3(256), 0, st, in, ld_in, out, ld_out, rows,
                       cols, u, inv_s, safe, V);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnr_cross_entropy_bwd_rows_f32(const float* logits, const int64_t* targets, int masked, int64_t ignore_index,
                                               const float* lse_row, const float* u, float* dlogits, int64_t rows, int V,
                                               void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && targets && lse_row && u && dlogits && V > 0 && rows > 0, "pdnr_cross_entropy_bwd_rows_f32: bad arguments");
  pdn_count(PDN_CNT_ROW_LOSS);
  hipStream_t st = (hipStream_t)stream;
  if (rce_reg_row_ok(V, logits, dlogits)) {
    hipLaunchKernelGGL(rce_bwd_reg_kernel, dim3(rce_reg_grid(rows)), dim3(1024), 0, st, logits, targets, masked, ignore_index,
                       lse_row, u, dlogits, rows, V);
  } else {
    const int g = (int)(rows < 65535 ? rows : 65535);
    hipLaunchKernelGGL(rce_bwd_rows_kernel, dim3(g), dim3(256), 0, st, logits, targets, masked, ignore_index, lse_row, u, dlogits,
                       rows, V);
  }
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnr_linear_ce_finish_rows_f32(const float* logits, int64_t ldl, float* lse, const int64_t* targets, int masked,
                                              int64_t ignore_index, int64_t rows, int V, float* loss_row, int64_t* targets_safe,
                                              int* err_flag, void* stream) {
  PDN_CHECK_ARG(rows > 0 && V > 0 && ldl >= V, "pdnr_linear_ce_finish_rows_f32: empty input");
  PDN_CHECK_ARG(logits && lse && targets && loss_row && targets_safe && err_flag, "pdnr_linear_ce_finish_rows_f32: null operand");
  pdn_count(PDN_CNT_ROW_LOSS);
  hipLaunchKernelGGL(rce_finish_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, ldl,
                     lse, targets, masked, ignore_index, rows, V, loss_row, targets_safe, err_flag);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnr_scale_rows_f32(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t rows, int cols,
                                   const float* u, const float* inv_s, const int64_t* targets_safe, int V, void* stream) {
  if (rows == 0 || cols == 0) return PDN_OK;
  PDN_CHECK_ARG(in && out && u && targets_safe && rows > 0 && cols > 0 && ld_in >= cols && ld_out >= cols,
                "pdnr_scale_rows_f32: bad arguments");
  pdn_count(PDN_CNT_ROW_LOSS);
  return rce_scale_rows(in, ld_in, out, ld_out, rows, cols, u, inv_s, targets_safe, V, (hipStream_t)stream);
}

extern "C" int pdnr_abs_max_rows_f32(const float* u, const int64_t* targets_safe, int V, int64_t rows, float* s_out,
                                     void* stream) {
  PDN_CHECK_ARG(u && targets_safe && s_out && rows >= 0, "pdnr_abs_max_rows_f32: bad arguments");
  pdn_count(PDN_CNT_ROW_LOSS);
  hipLaunchKernelGGL(rce_abs_max_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, u, targets_safe, V, rows, s_out);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnr_weighted_colsum_f32(const float* logits, int64_t ldl, const float* lse_masked, const int64_t* targets_safe,
                                        const float* u, int64_t rows, int V, float* dbias, float db_beta, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  PDN_CHECK_ARG(logits && lse_masked && targets_safe && u && dbias && rows > 0 && V > 0 && ldl >= V,
                "pdnr_weighted_colsum_f32: bad arguments");
  pdn_count(PDN_CNT_ROW_LOSS);
  return rce_colsum(logits, ldl, lse_masked, targets_safe, u, rows, V, dbias, db_beta, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

extern "C" int pdnr_linear_ce_backward_rows_f32(const float* x, int64_t ldx, const float* logits, const float* lse_masked,
                                                const int64_t* targets_safe, const float* u, const float* W, float* dx,
                                                float* dx_deferred, float* dW, float dw_beta, float* dbias, float db_beta,
                                                float* xs, float* s_out, int64_t rows, int V, int in_features, void* workspace,
                                                int64_t workspace_bytes, void* colsum_workspace,
                                                int64_t colsum_workspace_bytes, void* stream) {
  if (rows == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(x && logits && lse_masked && targets_safe && u && W, "pdnr_linear_ce_backward_rows_f32: null operand");
  PDN_CHECK_ARG(!(dx && dx_deferred), "pdnr_linear_ce_backward_rows_f32: dx and dx_deferred are exclusive");
  PDN_CHECK_ARG(!dW || (xs && s_out && (((uintptr_t)xs & 15) == 0)),
                "pdnr_linear_ce_backward_rows_f32: dW needs the aligned scratch xs and s_out");
  pdn_count(PDN_CNT_ROW_LOSS);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (dbias) {
    // first: its workspace may be the products'
    rc = rce_colsum(logits, V, lse_masked, targets_safe, u, rows, V, dbias, db_beta, colsum_workspace, colsum_workspace_bytes, st);
    if (rc) return rc;
  }
  if (dx) {
    rc = pdn_linear_ce_backward_f32(x, ldx, logits, lse_masked, targets_safe, 1.f, nullptr, W, dx, nullptr, nullptr, 0.f, nullptr,
                                    0.f, rows, V, in_features, workspace, workspace_bytes, stream);
    if (rc) return rc;
    rc = rce_scale_rows(dx, in_features, dx, in_features, rows, in_features, u, nullptr, targets_safe, V, st);
    if (rc) return rc;
  }
  if (dx_deferred) {
    rc = rce_scale_rows(dx_deferred, in_features, dx_deferred, in_features, rows, in_features, u, nullptr, targets_safe, V, st);
    if (rc) return rc;
  }
  if (dW) {
    hipLaunchKernelGGL(rce_abs_max_kernel, dim3(1), dim3(1024), 0, st, u, targets_safe, V, rows, s_out);
    PDN_LAUNCH_CHECK();
    rc = rce_scale_rows(x, ldx, xs, in_features, rows, in_features, u, s_out + 1, targets_safe, V, st);
    if (rc) return rc;
    rc = pdn_linear_ce_backward_f32(xs, in_features, logits, lse_masked, targets_safe, 1.f, s_out, W, nullptr, nullptr, dW,
                                    dw_beta, nullptr, 0.f, rows, V, in_features, workspace, workspace_bytes, stream);
    if (rc) return rc;
  }
  return PDN_OK;
}
