// Cross entropy with ignore_index (include/pdn_loss.h, prefix pdnl_): the masked forms of the unfused cross entropy
// (csrc/fused.hip) and of the lm_head + loss node (csrc/gemm.hip: pdn_linear_ce_backward_f32).  They extend
// nn/functional.py:364-381; the reference has no counterpart.  Statement: pydynet_amd/core/fused/masked_loss.py.
//
//   valid[n] = targets[n] != ignore_index;  count = sum(valid);  factor = mean ? (count ? 1 / count : 0) : 1
//   loss = factor * sum over valid rows of (lse[n] - logits[n][t[n]])
//   dlogits[n] = valid[n] ? (softmax(logits[n]) - onehot(t[n])) * factor * upstream : 0
//
// The count and the factor live on the device (stats[0], stats[1]): the host never learns them, so a captured step follows a
// targets buffer whose mask changes between replays.  Every reduction here runs in one workgroup in a fixed order.
// The lm_head node keeps its products (csrc/gemm_outres.hip, lm_head_dx_split.hip, lm_head_dw_split.hip) as they are: the
// finish kernel hands them an lse of +inf and a target of V for every ignored row, so that both dlogits terms
// (exp(logit - lse), [column == target]) are exactly 0 there; the input-gradient kernels subtract a gathered W[:, clamp(target)],
// so their rows of ignored tokens are set to 0 afterwards (pdnl_linear_ce_backward_f32).
#include "common.h"

#define MCE_REG_MAX_V 32768      // 1024 threads x 8 float4 held in registers (CE_REG_MAX_V of csrc/fused.hip)

extern "C" int pdn_linear_ce_backward_f32(const float* x, int64_t ldx, const float* logits, const float* lse,
                                          const int64_t* targets, float gscale, const float* upstream, const float* W, float* dx,
                                          const float* dx_residual, float* dW, float dw_beta, float* dbias, float db_beta,
                                          int64_t rows, int V, int in_features, void* workspace, int64_t workspace_bytes,
                                          void* stream);

static inline int mce_stream_grid(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
static inline bool mce_reg_row_ok(int V, const void* a, const void* b) {
  return V >= 4096 && V % 4 == 0 && V <= MCE_REG_MAX_V && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
}
static inline int mce_reg_grid(int64_t rows) { return (int)(rows < 256 ? rows : 256); }

// ---- count, factor and the loss: one workgroup, fixed order --------------------------------------------------------------
// targets != null: stats[0] = count, stats[1] = factor are written (else read); loss_row != null: loss_out = factor * sum.
// A row counts when its target differs from `ignore` (for the sanitised targets of the lm_head node: ignore = V).
__global__ __launch_bounds__(1024) void mce_reduce_kernel(const int64_t* __restrict__ targets, int64_t ignore,
                                                           const float* __restrict__ loss_row, int64_t rows, int mean,
                                                           float* __restrict__ stats, float* __restrict__ loss_out) {
  __shared__ float red[16];
  __shared__ int cnt[16];
  __shared__ float factor_s;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (targets) {
    int c = 0;
    for (int64_t i = tid; i < rows; i += 1024) c += targets[i] != ignore ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wid] = c;
    __syncthreads();
    if (tid == 0) {
      int64_t total = 0;
      for (int i = 0; i < 16; ++i) total += cnt[i];
      const float f = mean ? (total > 0 ? 1.f / (float)total : 0.f) : 1.f;
      stats[0] = (float)total;
      stats[1] = f;
      factor_s = f;
    }
  } else if (tid == 0) {
    factor_s = stats[1];
  }
  __syncthreads();
  if (!loss_row) return;
  float s = 0.f;
  for (int64_t i = tid; i < rows; i += 1024) s += loss_row[i];
  s = block_sum(s, red);
  if (tid == 0) loss_out[0] = s * factor_s;
}

// ---- unfused node, generic rows: one workgroup per row, the row re-read from L2 (ce_fwd_bwd_kernel of csrc/fused.hip) ----
template <bool WRITE>
__global__ void mce_row_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt, int64_t ignore,
                               float* __restrict__ loss_row, float* __restrict__ lse_row, float* __restrict__ dx,
                               const float* __restrict__ stats, int64_t rows, int V, int* __restrict__ err) {
  __shared__ float red[16];
  const float gscale = WRITE ? stats[1] : 1.f;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * (int64_t)V;
    float* dr = WRITE ? dx + row * (int64_t)V : nullptr;
    int64_t t = tgt[row];
    if (t == ignore) {                              // (uniform over the workgroup)
      if (WRITE)
        for (int c = threadIdx.x; c < V; c += blockDim.x) dr[c] = 0.f;
      if (threadIdx.x == 0) { lse_row[row] = 0.f; loss_row[row] = 0.f; }
      continue;
    }
    if (t < 0 || t >= V) { if (threadIdx.x == 0) *err = 1; t = 0; }
    const int n4 = ((((uintptr_t)xr | (uintptr_t)dr) & 15) == 0) ? V >> 2 : 0;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
    for (int c = n4 * 4 + threadIdx.x; c < V; c += blockDim.x) m = fmaxf(m, xr[c]);
    m = block_max(m, red);
    float s = 0.f;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      s += (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
    }
    for (int c = n4 * 4 + threadIdx.x; c < V; c += blockDim.x) s += expf(xr[c] - m);
    s = block_sum(s, red);
    const float lse = logf(s) + m;
    if (threadIdx.x == 0) {
      lse_row[row] = lse;
      loss_row[row] = lse - xr[t];
    }
    if (WRITE) {
      for (int i = threadIdx.x; i < n4; i += blockDim.x) {
        const float4 v = reinterpret_cast<const float4*>(xr)[i];
        float4 r;
        r.x = expf(v.x - lse); r.y = expf(v.y - lse); r.z = expf(v.z - lse); r.w = expf(v.w - lse);
        const int c = 4 * i;
        if (t >= c && t < c + 4) {
          if (t == c) r.x -= 1.f; else if (t == c + 1) r.y -= 1.f;
          else if (t == c + 2) r.z -= 1.f; else r.w -= 1.f;
        }
        r.x *= gscale; r.y *= gscale; r.z *= gscale; r.w *= gscale;
        reinterpret_cast<float4*>(dr)[i] = r;
      }
      for (int c = n4 * 4 + threadIdx.x; c < V; c += blockDim.x)
        dr[c] = (expf(xr[c] - lse) - (c == t ? 1.f : 0.f)) * gscale;
    }
    __syncthreads();                  // red is rewritten by the next row
  }
}

// ---- unfused node, the row held in registers (ce_fwd_bwd_reg_kernel of csrc/fused.hip): 4096 <= V <= 32768, V % 4 == 0 ---
// One 1024-thread workgroup walks rows; the next row is fetched while the current one is reduced and written.  An ignored
// row is fetched like any other (the stream stays one row ahead) and then only zero-filled.
template <bool COLSUM, bool WRITE>
__global__ __launch_bounds__(1024) void mce_reg_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                        int64_t ignore, float* __restrict__ loss_row,
                                                        float* __restrict__ lse_row, float* __restrict__ dx,
                                                        const float* __restrict__ stats, int64_t rows, int V,
                                                        int* __restrict__ err, float* __restrict__ colsum_part) {
  constexpr int NV = MCE_REG_MAX_V / 4 / 1024;     // float4 per thread
  __shared__ float red[16];
  __shared__ float xt_s;
  const int n4 = V >> 2, tid = threadIdx.x;
  const float gscale = WRITE ? stats[1] : 1.f;
  float4 cur[NV], nxt[NV], cs[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    cs[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    nxt[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  int64_t row = blockIdx.x;
  if (row < rows) {
    const float4* xr = reinterpret_cast<const float4*>(x + row * (int64_t)V);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      if (i < n4) nxt[j] = xr[i];
    }
  }
  for (; row < rows; row += gridDim.x) {
    int64_t t = tgt[row];
    const bool ign = t == ignore;                   // (uniform over the workgroup)
    if (!ign && (t < 0 || t >= V)) { if (tid == 0) *err = 1; t = 0; }
    const int t4 = ign ? -1 : (int)(t >> 2), tc = (int)(t & 3);
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      cur[j] = nxt[j];
      if (i < n4) {
        const float4 v = cur[j];
        m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        if (i == t4) xt_s = tc == 0 ? v.x : (tc == 1 ? v.y : (tc == 2 ? v.z : v.w));
      }
    }
    const int64_t nrow = row + gridDim.x;
    if (nrow < rows) {
      const float4* xn = reinterpret_cast<const float4*>(x + nrow * (int64_t)V);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int i = tid + 1024 * j;
        if (i < n4) nxt[j] = xn[i];
      }
    }
    if (ign) {
      if (tid == 0) { lse_row[row] = 0.f; loss_row[row] = 0.f; }
      if (WRITE) {
        float4* dz = reinterpret_cast<float4*>(dx + row * (int64_t)V);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const int i = tid + 1024 * j;
          if (i < n4) dz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      continue;                                     // nothing of this row touched red / xt_s
    }
    m = block_max(m, red);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      if (i < n4) {
        float4 e;
        e.x = expf(cur[j].x - m); e.y = expf(cur[j].y - m); e.z = expf(cur[j].z - m); e.w = expf(cur[j].w - m);
        cur[j] = e;
        s += (e.x + e.y) + (e.z + e.w);
      }
    }
    s = block_sum(s, red);            // (its barriers also publish xt_s)
    const float lse = logf(s) + m;
    const float inv = 1.f / s;
    if (tid == 0) {
      lse_row[row] = lse;
      loss_row[row] = lse - xt_s;
    }
    if (WRITE) {
      float4* dr = reinterpret_cast<float4*>(dx + row * (int64_t)V);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int i = tid + 1024 * j;
        if (i < n4) {
          float4 r;
          r.x = cur[j].x * inv; r.y = cur[j].y * inv; r.z = cur[j].z * inv; r.w = cur[j].w * inv;
          if (i == t4) {
            if (tc == 0) r.x -= 1.f; else if (tc == 1) r.y -= 1.f;
            else if (tc == 2) r.z -= 1.f; else r.w -= 1.f;
          }
          r.x *= gscale; r.y *= gscale; r.z *= gscale; r.w *= gscale;
          dr[i] = r;
          if (COLSUM) { cs[j].x += r.x; cs[j].y += r.y; cs[j].z += r.z; cs[j].w += r.w; }
        }
      }
    }
    __syncthreads();                  // xt_s / red are rewritten by the next row
  }
  if (COLSUM) {
    float4* part = reinterpret_cast<float4*>(colsum_part + (int64_t)blockIdx.x * V);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      if (i < n4) part[i] = cs[j];
    }
  }
}
// the workgroups' partial rows added up, one thread per column, parts in their order
__global__ __launch_bounds__(256) void mce_colsum_kernel(const float* __restrict__ part, int nb, int V, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= V) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += part[(int64_t)b * V + c];
  out[c] = s;
}

// ---- unfused node, backward on its own (pdn_cross_entropy_bwd_f32's case) -------------------------------------------------
__global__ void mce_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt, int64_t ignore,
                               const float* __restrict__ lse_row, const float* __restrict__ upstream,
                               const float* __restrict__ stats, float* __restrict__ dx, int64_t rows, int V) {
  const float gs = stats[1] * (upstream ? upstream[0] : 1.f);
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * (int64_t)V;
    float* dr = dx + row * (int64_t)V;
    const int64_t t = tgt[row];
    if (t == ignore) {
      for (int c = threadIdx.x; c < V; c += blockDim.x) dr[c] = 0.f;
      continue;
    }
    const float lse = lse_row[row];
    for (int c = threadIdx.x; c < V; c += blockDim.x) dr[c] = (expf(xr[c] - lse) - (c == t ? 1.f : 0.f)) * gs;
  }
}

// ---- lm_head node: the finish after the projection -------------------------------------------------------------------------
// per row: loss_row = lse - logit[target] (0 when ignored); targets_safe = target (V when ignored, 0 for a bad one, flagged);
// lse = +inf when ignored
__global__ void mce_finish_rows_kernel(const float* __restrict__ logits, int64_t ldl, float* __restrict__ lse,
                                       const int64_t* __restrict__ tgt, int64_t ignore, int64_t rows, int V,
                                       float* __restrict__ loss_row, int64_t* __restrict__ safe, int* __restrict__ err) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= rows) return;
  int64_t t = tgt[r];
  if (t == ignore) {
    loss_row[r] = 0.f;
    safe[r] = V;
    lse[r] = INFINITY;
    return;
  }
  if (t < 0 || t >= V) { *err = 1; t = 0; }
  loss_row[r] = lse[r] - logits[r * ldl + t];
  safe[r] = t;
}
// stats[2] = upstream * factor: the device scalar both products of the backward take as their upstream gradient
__global__ void mce_upstream_kernel(const float* __restrict__ upstream, float* __restrict__ stats) {
  stats[2] = (upstream ? upstream[0] : 1.f) * stats[1];
}
// rows of ignored tokens set to 0, the others multiplied by *scale (scale null or 1: left as they are)
template <bool VEC>
__global__ void mce_mask_rows_kernel(float* __restrict__ x, int64_t ld, int64_t rows, int cols,
                                     const int64_t* __restrict__ safe, int V, const float* __restrict__ scale) {
  const float s = scale ? scale[0] : 1.f;
  const int per = VEC ? cols >> 2 : cols;
  const int64_t total = rows * per, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / per;
    const int c = (int)(i - r * per);
    const bool keep = safe[r] != V;
    if (keep && s == 1.f) continue;
    if (VEC) {
      float4* p = reinterpret_cast<float4*>(x + r * ld) + c;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (keep) { v = *p; v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
      *p = v;
    } else {
      float* p = x + r * ld + c;
      *p = keep ? *p * s : 0.f;
    }
  }
}

// =============================================================================================================================
extern "C" int64_t pdnl_cross_entropy_colsum_workspace_bytes(int64_t rows, int V) {
  if (!(V >= 4096 && V % 4 == 0 && V <= MCE_REG_MAX_V) || rows <= 0) return 0;
  return (int64_t)mce_reg_grid(rows) * V * 4;
}

static void mce_launch_rows(bool write, const float* logits, const int64_t* targets, int64_t ignore, int64_t rows, int V,
                            float* loss_row, float* lse_row, float* dlogits, const float* stats, float* colsum_part,
                            int* err_flag, hipStream_t st) {
  if (mce_reg_row_ok(V, logits, write ? dlogits : logits)) {
    const dim3 g(mce_reg_grid(rows)), b(1024);
    if (!write)
      hipLaunchKernelGGL((mce_reg_kernel<false, false>), g, b, 0, st, logits, targets, ignore, loss_row, lse_row,
                         (float*)nullptr, stats, rows, V, err_flag, (float*)nullptr);
    else if (colsum_part)
      hipLaunchKernelGGL((mce_reg_kernel<true, true>), g, b, 0, st, logits, targets, ignore, loss_row, lse_row, dlogits, stats,
                         rows, V, err_flag, colsum_part);
    else
      hipLaunchKernelGGL((mce_reg_kernel<false, true>), g, b, 0, st, logits, targets, ignore, loss_row, lse_row, dlogits, stats,
                         rows, V, err_flag, (float*)nullptr);
    return;
  }
  // long rows: few, fat workgroups so the rows in flight stay within L2 for the re-read passes (pdn_cross_entropy_fwd_f32)
  const int threads = V >= 4096 ? 1024 : 256;
  const int g = (int)(V >= 4096 ? (rows < 512 ? rows : 512) : (rows < 65535 ? rows : 65535));
  if (write)
    hipLaunchKernelGGL((mce_row_kernel<true>), dim3(g), dim3(threads), 0, st, logits, targets, ignore, loss_row, lse_row, dlogits,
                       stats, rows, V, err_flag);
  else
    hipLaunchKernelGGL((mce_row_kernel<false>), dim3(g), dim3(threads), 0, st, logits, targets, ignore, loss_row, lse_row,
                       (float*)nullptr, stats, rows, V, err_flag);
}

extern "C" int pdnl_cross_entropy_fwd_f32(const float* logits, const int64_t* targets, int64_t ignore_index, int64_t rows, int V,
                                          int mean, float* loss_row, float* lse_row, float* loss_out, float* stats,
                                          int* err_flag, void* stream) {
  PDN_CHECK_ARG(rows > 0 && V > 0, "pdnl_cross_entropy_fwd_f32: empty input");
  PDN_CHECK_ARG(logits && targets && loss_row && lse_row && loss_out && stats && err_flag, "pdnl_cross_entropy_fwd_f32: null operand");
  hipStream_t st = (hipStream_t)stream;
  mce_launch_rows(false, logits, targets, ignore_index, rows, V, loss_row, lse_row, nullptr, stats, nullptr, err_flag, st);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(mce_reduce_kernel, dim3(1), dim3(1024), 0, st, targets, ignore_index, (const float*)loss_row, rows, mean,
                     stats, loss_out);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnl_cross_entropy_fwd_bwd_f32(const float* logits, const int64_t* targets, int64_t ignore_index, int64_t rows,
                                              int V, int mean, float* loss_row, float* lse_row, float* loss_out, float* stats,
                                              float* dlogits, float* dlogits_colsum, void* workspace, int64_t workspace_bytes,
                                              int* err_flag, void* stream) {
  PDN_CHECK_ARG(rows > 0 && V > 0, "pdnl_cross_entropy_fwd_bwd_f32: empty input");
  PDN_CHECK_ARG(logits && targets && loss_row && lse_row && loss_out && stats && dlogits && err_flag,
                "pdnl_cross_entropy_fwd_bwd_f32: null operand");
  hipStream_t st = (hipStream_t)stream;
  if (dlogits_colsum) {
    if (!mce_reg_row_ok(V, logits, dlogits)) {
      pdn_set_error("pdnl_cross_entropy_fwd_bwd_f32: fused column sums need 4096 <= V <= %d, V %% 4 == 0, aligned rows", MCE_REG_MAX_V);
      return PDN_EUNSUPPORTED;
    }
    if (!workspace || workspace_bytes < pdnl_cross_entropy_colsum_workspace_bytes(rows, V)) {
      pdn_set_error("pdnl_cross_entropy_fwd_bwd_f32: workspace too small");
      return PDN_EWORKSPACE;
    }
  }
  // the factor first: the rows are written already scaled by it
  hipLaunchKernelGGL(mce_reduce_kernel, dim3(1), dim3(1024), 0, st, targets, ignore_index, (const float*)nullptr, rows, mean, stats,
                     (float*)nullptr);
  PDN_LAUNCH_CHECK();
  mce_launch_rows(true, logits, targets, ignore_index, rows, V, loss_row, lse_row, dlogits, stats,
                  dlogits_colsum ? (float*)workspace : nullptr, err_flag, st);
  PDN_LAUNCH_CHECK();
  if (dlogits_colsum) {
    hipLaunchKernelGGL(mce_colsum_kernel, dim3((V + 255) / 256), dim3(256), 0, st, (const float*)workspace, mce_reg_grid(rows), V,
                       dlogits_colsum);
    PDN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(mce_reduce_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)nullptr, (int64_t)0, (const float*)loss_row,
                     rows, mean, stats, loss_out);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnl_cross_entropy_bwd_f32(const float* logits, const int64_t* targets, int64_t ignore_index, const float* lse_row,
                                          const float* upstream, const float* stats, float* dlogits, int64_t rows, int V,
                                          void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && targets && lse_row && stats && dlogits && V > 0 && rows > 0, "pdnl_cross_entropy_bwd_f32: bad arguments");
  const int g = (int)(rows < 65535 ? rows : 65535);
  hipLaunchKernelGGL(mce_bwd_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, logits, targets, ignore_index, lse_row, upstream,
                     stats, dlogits, rows, V);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnl_linear_ce_finish_f32(const float* logits, int64_t ldl, float* lse, const int64_t* targets, int64_t ignore_index,
                                         int64_t rows, int V, int mean, float* loss_row, float* loss_out, float* stats,
                                         int64_t* targets_safe, int* err_flag, void* stream) {
  PDN_CHECK_ARG(rows > 0 && V > 0 && ldl >= V, "pdnl_linear_ce_finish_f32: empty input");
  PDN_CHECK_ARG(logits && lse && targets && loss_row && loss_out && stats && targets_safe && err_flag,
                "pdnl_linear_ce_finish_f32: null operand");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mce_finish_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, logits, ldl, lse, targets,
                     ignore_index, rows, V, loss_row, targets_safe, err_flag);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(mce_reduce_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)targets_safe, (int64_t)V,
                     (const float*)loss_row, rows, mean, stats, loss_out);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

static int mce_mask_rows(float* x, int64_t ld, int64_t rows, int cols, const int64_t* safe, int V, const float* scale,
                         hipStream_t st) {
  const bool vec = cols % 4 == 0 && ld % 4 == 0 && (((uintptr_t)x & 15) == 0);
  const int64_t total = rows * (vec ? cols / 4 : cols);
  if (vec)
    hipLaunchKernelGGL((mce_mask_rows_kernel<true>), dim3(mce_stream_grid(total)), dim3(256), 0, st, x, ld, rows, cols, safe, V, scale);
  else
    hipLaunchKernelGGL((mce_mask_rows_kernel<false>), dim3(mce_stream_grid(total)), dim3(256), 0, st, x, ld, rows, cols, safe, V, scale);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnl_linear_ce_backward_f32(const float* x, int64_t ldx, const float* logits, const float* lse_masked,
                                           const int64_t* targets_safe, float* stats, const float* upstream, const float* W,
                                           float* dx, float* dx_deferred, float* dW, float dw_beta, float* dbias, float db_beta,
                                           int64_t rows, int V, int in_features, void* workspace, int64_t workspace_bytes,
                                           void* stream) {
  if (rows == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(x && logits && lse_masked && targets_safe && stats && W, "pdnl_linear_ce_backward_f32: null operand");
  PDN_CHECK_ARG(!(dx && dx_deferred), "pdnl_linear_ce_backward_f32: dx and dx_deferred are exclusive");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mce_upstream_kernel, dim3(1), dim3(1), 0, st, upstream, stats);
  PDN_LAUNCH_CHECK();
  if (dx || dW || dbias) {
    // the products as they are: gscale 1, the upstream scalar carries the factor; no residual fold (the rows set to 0 below
    // would lose it)
    const int rc = pdn_linear_ce_backward_f32(x, ldx, logits, lse_masked, targets_safe, 1.f, stats + 2, W, dx, nullptr, dW, dw_beta,
                                              dbias, db_beta, rows, V, in_features, workspace, workspace_bytes, stream);
    if (rc) return rc;
  }
  if (dx) return mce_mask_rows(dx, in_features, rows, in_features, targets_safe, V, nullptr, st);
  if (dx_deferred) return mce_mask_rows(dx_deferred, in_features, rows, in_features, targets_safe, V, stats + 2, st);
  return PDN_OK;
}
