// Cross entropy with label_smoothing and z_loss (include/pdn_smoothloss.h, prefix pdnz_): the smoothed forms of the unfused
// cross entropy (csrc/fused.hip, csrc/masked_loss.hip, csrc/row_loss.hip) and the terms that go AROUND the lm_head + loss
// node's products.  They extend nn/functional.py:364-381; the reference has no counterpart.  Statement:
// pydynet_amd/core/fused/smooth_loss.py.
//
//   valid[n] = !masked || targets[n] != ignore_index;   lse = logsumexp(z[n]);   a = 1 + 2 lam lse
//   row[n]   = valid ? lse - (1 - eps) z[n][t] - eps mean_v z[n] + lam lse^2 : 0
//   dz[n]    = valid ? u[n] (a softmax(z[n]) - (1 - eps) onehot(t) - eps / V) : 0
//            = u' (softmax - onehot) + c onehot - e          u' = u a,  c = u (2 lam lse + eps),  e = u eps / V
//
// The lm_head products (csrc/gemm_outres.hip, lm_head_dx_split.hip, lm_head_dw_split.hip) and the reduction='none' backward
// around them (pdnr_linear_ce_backward_rows_f32) stay as they are and run under the upstream vector u'.  The two other terms
// need no pass over the logits: mean_v z[n] = (x[n] . wsum + bsum) / V with wsum the row sums of W; the c term adds one
// weight column to a dx row and one x row to a dW column; the e term is rank 1.  The sums of x rows into the dW column of
// their class have a fixed order without a sort: a workgroup owns a contiguous range of classes with an fp32 accumulator in
// LDS, walks ALL sanitised targets in row order and adds the rows that fall into its range.  Every reduction here has a fixed
// order, nothing is allocated, nothing is read back.
#include "common.h"

#define ZCE_REG_MAX_V 32768      // 1024 threads x 8 float4 held in registers (MCE_REG_MAX_V of csrc/masked_loss.hip)
#define ZCE_LDS_FLOATS 14336     // the class-owned accumulator: 56 KiB of the 64 KiB a workgroup may take without opting in (4 KiB more are static)
#define ZCE_MAX_CLASSES 128      // classes per workgroup at most

static inline int zce_stream_grid(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
static inline bool zce_reg_row_ok(int V, const void* a, const void* b) {
  return V >= 4096 && V % 4 == 0 && V <= ZCE_REG_MAX_V && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
}
static inline int zce_reg_grid(int64_t rows) { return (int)(rows < 256 ? rows : 256); }

// ---- count, factor and the loss: one workgroup, fixed order (mce_reduce_kernel of csrc/masked_loss.hip with the masked flag) --
__global__ __launch_bounds__(1024) void zce_reduce_kernel(const int64_t* __restrict__ targets, int masked, int64_t ignore,
                                                           const float* __restrict__ loss_row, int64_t rows, int mean,
                                                           float* __restrict__ stats, float* __restrict__ loss_out) {
  __shared__ float red[16];
  __shared__ int cnt[16];
  __shared__ float factor_s;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int c = 0;
  for (int64_t i = tid; i < rows; i += 1024) c += (!masked || targets[i] != ignore) ? 1 : 0;
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
  __syncthreads();
  float s = 0.f;
  for (int64_t i = tid; i < rows; i += 1024) s += loss_row[i];
  s = block_sum(s, red);
  if (tid == 0) loss_out[0] = s * factor_s;
}

// the row's value from its three sums; thread 0 of the workgroup
__device__ __forceinline__ void zce_store_row(float m, float s, float sz, float xt, int V, float eps, float lam, float* lse_out,
                                              float* loss_out) {
  const float lse = logf(s) + m;
  *lse_out = lse;
  *loss_out = lse - (1.f - eps) * xt - eps * (sz / (float)V) + lam * lse * lse;
}

// ---- unfused forward, streamed rows: one workgroup per row, ONE pass -- every thread keeps a running (max, sum of
// exponentials, sum) over its elements, float4 where the row's address allows it ---------------------------------------------
__global__ void zce_fwd_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt, int masked, int64_t ignore,
                                    float* __restrict__ loss_row, float* __restrict__ lse_row, int64_t rows, int V, float eps,
                                    float lam, int* __restrict__ err) {
  __shared__ float red[16];
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * (int64_t)V;
    int64_t t = tgt[row];
    if (masked && t == ignore) {                    // (uniform over the workgroup)
      if (threadIdx.x == 0) { lse_row[row] = 0.f; loss_row[row] = 0.f; }
      continue;
    }
    if (t < 0 || t >= V) { if (threadIdx.x == 0) *err = 1; t = 0; }
    const int n4 = (((uintptr_t)xr & 15) == 0) ? V >> 2 : 0;
    float m = -INFINITY, s = 0.f, sz = 0.f;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      const float nm = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
      s = s * expf(m - nm) + ((expf(v.x - nm) + expf(v.y - nm)) + (expf(v.z - nm) + expf(v.w - nm)));
      sz += (v.x + v.y) + (v.z + v.w);
      m = nm;
    }
    for (int c = n4 * 4 + threadIdx.x; c < V; c += blockDim.x) {
      const float v = xr[c];
      const float nm = fmaxf(m, v);
      s = s * expf(m - nm) + expf(v - nm);
      sz += v;
      m = nm;
    }
    const float mm = block_max(m, red);
    s = m == -INFINITY ? 0.f : s * expf(m - mm);    // (a thread without an element)
    s = block_sum(s, red);
    sz = block_sum(sz, red);
    if (threadIdx.x == 0) zce_store_row(mm, s, sz, xr[t], V, eps, lam, lse_row + row, loss_row + row);
    __syncthreads();                  // red is rewritten by the next row
  }
}

// ---- unfused forward, the row held in registers (mce_reg_kernel of csrc/masked_loss.hip): 4096 <= V <= 32768, V % 4 == 0,
// aligned rows.  One 1024-thread workgroup walks rows; the next row is fetched while the current one is reduced. -----------------
__global__ __launch_bounds__(1024) void zce_fwd_reg_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                            int masked, int64_t ignore, float* __restrict__ loss_row,
                                                            float* __restrict__ lse_row, int64_t rows, int V, float eps,
                                                            float lam, int* __restrict__ err) {
  constexpr int NV = ZCE_REG_MAX_V / 4 / 1024;     // float4 per thread
  __shared__ float red[16];
  __shared__ float xt_s;
  const int n4 = V >> 2, tid = threadIdx.x;
  float4 cur[NV], nxt[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) nxt[j] = make_float4(0.f, 0.f, 0.f, 0.f);
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
    const bool ign = masked && t == ignore;         // (uniform over the workgroup)
    if (!ign && (t < 0 || t >= V)) { if (tid == 0) *err = 1; t = 0; }
    const int t4 = ign ? -1 : (int)(t >> 2), tc = (int)(t & 3);
    float m = -INFINITY, sz = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      cur[j] = nxt[j];
      if (i < n4) {
        const float4 v = cur[j];
        m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
        sz += (v.x + v.y) + (v.z + v.w);
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
      continue;                                     // nothing of this row touched red / xt_s
    }
    m = block_max(m, red);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      if (i < n4) s += (expf(cur[j].x - m) + expf(cur[j].y - m)) + (expf(cur[j].z - m) + expf(cur[j].w - m));
    }
    s = block_sum(s, red);            // (its barriers also publish xt_s)
    sz = block_sum(sz, red);
    if (tid == 0) zce_store_row(m, s, sz, xt_s, V, eps, lam, lse_row + row, loss_row + row);
    __syncthreads();                  // xt_s / red are rewritten by the next row
  }
}

// ---- unfused backward.  The row's upstream number: u[row], or upstream[0] * stats[1] (either NULL: 1) ------------------------
__device__ __forceinline__ float zce_upstream(const float* __restrict__ u, const float* __restrict__ upstream,
                                              const float* __restrict__ stats, int64_t row) {
  return u ? u[row] : (upstream ? upstream[0] : 1.f) * (stats ? stats[1] : 1.f);
}
__device__ __forceinline__ float zce_dz(float v, float lse, float a, bool hit, float hot, float uni, float g) {
  return (a * expf(v - lse) - (hit ? hot : 0.f) - uni) * g;
}

__global__ void zce_bwd_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt, int masked, int64_t ignore,
                                    const float* __restrict__ lse_row, const float* __restrict__ u,
                                    const float* __restrict__ upstream, const float* __restrict__ stats, float eps, float lam,
                                    float* __restrict__ dx, int64_t rows, int V) {
  const float hot = 1.f - eps, uni = eps / (float)V;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* xr = x + row * (int64_t)V;
    float* dr = dx + row * (int64_t)V;
    const int64_t t = tgt[row];
    const bool valid = !masked || t != ignore;      // (uniform over the workgroup)
    const float lse = lse_row[row];
    const float a = 1.f + 2.f * lam * lse;
    const float g = valid ? zce_upstream(u, upstream, stats, row) : 0.f;
    const int n4 = ((((uintptr_t)xr | (uintptr_t)dr) & 15) == 0) ? V >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 v = reinterpret_cast<const float4*>(xr)[i];
      const int c = 4 * i;
      float4 r;
      r.x = zce_dz(v.x, lse, a, t == c, hot, uni, g);
      r.y = zce_dz(v.y, lse, a, t == c + 1, hot, uni, g);
      r.z = zce_dz(v.z, lse, a, t == c + 2, hot, uni, g);
      r.w = zce_dz(v.w, lse, a, t == c + 3, hot, uni, g);
      reinterpret_cast<float4*>(dr)[i] = valid ? r : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int c = n4 * 4 + threadIdx.x; c < V; c += blockDim.x) {
      const float r = zce_dz(xr[c], lse, a, c == t, hot, uni, g);
      dr[c] = valid ? r : 0.f;
    }
  }
}

// the row passed through registers (rce_bwd_reg_kernel of csrc/row_loss.hip): the lse is saved, so nothing is reduced
__global__ __launch_bounds__(1024) void zce_bwd_reg_kernel(const float* __restrict__ x, const int64_t* __restrict__ tgt,
                                                            int masked, int64_t ignore, const float* __restrict__ lse_row,
                                                            const float* __restrict__ u, const float* __restrict__ upstream,
                                                            const float* __restrict__ stats, float eps, float lam,
                                                            float* __restrict__ dx, int64_t rows, int V) {
  constexpr int NV = ZCE_REG_MAX_V / 4 / 1024;     // float4 per thread
  const int n4 = V >> 2, tid = threadIdx.x;
  const float hot = 1.f - eps, uni = eps / (float)V;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t t = tgt[row];
    const bool valid = !masked || t != ignore;
    const float4* xr = reinterpret_cast<const float4*>(x + row * (int64_t)V);
    float4* dr = reinterpret_cast<float4*>(dx + row * (int64_t)V);
    float4 cur[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      cur[j] = i < n4 ? xr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float lse = lse_row[row];
    const float a = 1.f + 2.f * lam * lse;
    const float g = valid ? zce_upstream(u, upstream, stats, row) : 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = tid + 1024 * j;
      if (i < n4) {
        const int c = 4 * i;
        float4 r;
        r.x = zce_dz(cur[j].x, lse, a, t == c, hot, uni, g);
        r.y = zce_dz(cur[j].y, lse, a, t == c + 1, hot, uni, g);
        r.z = zce_dz(cur[j].z, lse, a, t == c + 2, hot, uni, g);
        r.w = zce_dz(cur[j].w, lse, a, t == c + 3, hot, uni, g);
        dr[i] = valid ? r : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
}

// ---- lm_head node: wsum[k] = sum_v W[k][v] for k < in_features, wsum[in_features] = sum_v bias[v] (0 without a bias): one
// workgroup per sum, a thread's elements in their order, then the workgroup's fixed tree ----------------------------------------
__global__ __launch_bounds__(256) void zce_weight_sums_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                               int in_features, int V, float* __restrict__ wsum) {
  __shared__ float red[16];
  const int k = blockIdx.x;
  const float* src = k < in_features ? W + (int64_t)k * V : bias;
  float s = 0.f;
  if (src) {
    const int n4 = (((uintptr_t)src & 15) == 0) ? V >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += 256) {
      const float4 v = reinterpret_cast<const float4*>(src)[i];
      s += (v.x + v.y) + (v.z + v.w);
    }
    for (int c = n4 * 4 + threadIdx.x; c < V; c += 256) s += src[c];
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) wsum[k] = s;
}

// ---- lm_head node: the finish after the projection (rce_finish_rows_kernel of csrc/row_loss.hip with the two terms): a wave
// per row, its lanes over the features of x[n] . wsum ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zce_finish_rows_kernel(const float* __restrict__ logits, int64_t ldl,
                                                               float* __restrict__ lse, const int64_t* __restrict__ tgt,
                                                               int masked, int64_t ignore, const float* __restrict__ x,
                                                               int64_t ldx, const float* __restrict__ wsum, int64_t rows, int V,
                                                               int in_features, float eps, float lam,
                                                               float* __restrict__ loss_row, int64_t* __restrict__ safe,
                                                               int* __restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t r = blockIdx.x * (int64_t)4 + (threadIdx.x >> 6); r < rows; r += stride) {
    int64_t t = tgt[r];
    if (masked && t == ignore) {                    // (uniform over the wave)
      if (lane == 0) { loss_row[r] = 0.f; safe[r] = V; lse[r] = INFINITY; }
      continue;
    }
    if (t < 0 || t >= V) { if (lane == 0) *err = 1; t = 0; }
    float dot = 0.f;
    if (eps != 0.f) {
      const float* xr = x + r * ldx;
      for (int k = lane; k < in_features; k += 64) dot += xr[k] * wsum[k];
      dot = wave_sum(dot);
    }
    if (lane == 0) {
      const float l = lse[r];
      const float zmean = eps != 0.f ? (dot + wsum[in_features]) / (float)V : 0.f;
      loss_row[r] = l - (1.f - eps) * logits[r * ldl + t] - eps * zmean + lam * l * l;
      safe[r] = t;
    }
  }
}

// ---- lm_head node: the row coefficients u' = u a, c = u (2 lam lse + eps), e = u eps / V; exactly 0 on ignored rows ----------
__global__ void zce_coefficients_kernel(const float* __restrict__ lse, const int64_t* __restrict__ safe,
                                        const float* __restrict__ u, const float* __restrict__ upstream,
                                        const float* __restrict__ stats, float eps, float lam, int64_t rows, int V,
                                        float* __restrict__ u_out, float* __restrict__ c_out, float* __restrict__ e_out) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const bool keep = safe[r] != V;
  const float g = keep ? zce_upstream(u, upstream, stats, r) : 0.f;
  const float zl = keep ? 2.f * lam * lse[r] : 0.f;
  u_out[r] = keep ? g * (1.f + zl) : 0.f;
  c_out[r] = keep ? g * (zl + eps) : 0.f;
  e_out[r] = keep ? g * (eps / (float)V) : 0.f;
}

// ---- lm_head node, dx: dx[n][k] += c[n] W[k][t[n]] - e[n] wsum[k]; rows of ignored tokens are left as they are (exactly 0) ----
__global__ void zce_dx_kernel(float* __restrict__ dx, const float* __restrict__ W, const float* __restrict__ wsum,
                              const int64_t* __restrict__ safe, const float* __restrict__ c, const float* __restrict__ e,
                              int64_t rows, int V, int in_features) {
  const int64_t total = rows * in_features, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / in_features;
    const int k = (int)(i - r * in_features);
    const int64_t t = safe[r];
    if (t == V) continue;
    float v = dx[i] + c[r] * W[(int64_t)k * V + t];
    if (e) v -= e[r] * wsum[k];
    dx[i] = v;
  }
}

// ---- lm_head node, the uniform term of dW and dbias: r[k] = sum_n e[n] x[n][k] (k == in_features: sum_n e[n]) in two stages,
// a slab of rows per workgroup row, a feature per thread, rows in their order; then the slabs in their order --------------------
__global__ __launch_bounds__(256) void zce_esum_part_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ e,
                                                             int64_t rows, int in_features, int64_t rows_per_slab,
                                                             float* __restrict__ part) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k > in_features) return;                      // (no barrier below)
  const int64_t r0 = blockIdx.y * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  float acc = 0.f;
  if (k < in_features) {
    for (int64_t r = r0; r < r1; ++r) acc += e[r] * x[r * ldx + k];
  } else {
    for (int64_t r = r0; r < r1; ++r) acc += e[r];
  }
  part[(int64_t)blockIdx.y * (in_features + 1) + k] = acc;
}
__global__ __launch_bounds__(256) void zce_esum_reduce_kernel(const float* __restrict__ part, int slabs, int in_features,
                                                               float* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k > in_features) return;
  float s = 0.f;
  for (int b = 0; b < slabs; ++b) s += part[(int64_t)b * (in_features + 1) + k];
  out[k] = s;
}

// ---- lm_head node, the target-column term of dW and dbias.  Workgroup b owns the classes [b * cpw, b * cpw + cpw) and an
// accumulator acc[class][feature] in LDS (feature in_features: the bias, x replaced by 1; rows of `ld` floats, ld odd).  It
// walks all sanitised targets, 256 rows at a time: every thread tests one row, the waves' ballots are published, and all
// threads then go through the rows that hit IN ROW ORDER, a thread adding c[n] x[n][k] for the features k it owns -- no two
// threads ever touch one accumulator, so the order of every sum is the row order.  An ignored row carries the target V, which
// lies in no range.  At the end the workgroup adds its columns to dW and dbias once, the uniform term r folded in. ---------------
__global__ __launch_bounds__(256) void zce_class_sums_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const int64_t* __restrict__ safe, const float* __restrict__ c,
                                                              const float* __restrict__ r, float* __restrict__ dW,
                                                              float* __restrict__ dbias, int64_t rows, int V, int in_features,
                                                              int cpw, int ld) {
  extern __shared__ float acc[];
  __shared__ unsigned long long hits[2][4];
  __shared__ int cls[2][256];
  __shared__ float coef[2][256];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int v0 = blockIdx.x * cpw;
  const int nv = V - v0 < cpw ? V - v0 : cpw;
  const int k_lo = dW ? 0 : in_features, k_hi = dbias ? in_features : in_features - 1;      // the features kept
  for (int i = tid; i < nv * ld; i += 256) acc[i] = 0.f;
  int p = 0;
  for (int64_t base = 0; base < rows; base += 256, p ^= 1) {
    const int64_t n = base + tid;
    const int64_t t = n < rows ? safe[n] : (int64_t)V;
    const bool hit = t >= v0 && t < v0 + nv;
    const unsigned long long mask = __ballot(hit);
    cls[p][tid] = hit ? (int)(t - v0) : 0;
    coef[p][tid] = hit ? c[n] : 0.f;
    if (lane == 0) hits[p][wid] = mask;
    __syncthreads();                  // (also orders the zero fill above; buffer p is rewritten two barriers from here)
    for (int w = 0; w < 4; ++w) {
      unsigned long long m = hits[p][w];
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int q = w * 64 + b;
        const float cn = coef[p][q];
        const float* xr = x + (base + q) * ldx;
        float* a = acc + cls[p][q] * ld;
        for (int k = k_lo + tid; k <= k_hi; k += 256) a[k] += cn * (k < in_features ? xr[k] : 1.f);
      }
    }
  }
  __syncthreads();
  if (dW) {
    for (int i = tid; i < in_features * nv; i += 256) {
      const int k = i / nv, j = i - k * nv;
      float* o = dW + (int64_t)k * V + v0 + j;
      *o += acc[j * ld + k] - (r ? r[k] : 0.f);
    }
  }
  if (dbias) {
    for (int j = tid; j < nv; j += 256) dbias[v0 + j] += acc[j * ld + in_features] - (r ? r[in_features] : 0.f);
  }
}

// =============================================================================================================================
static inline int zce_acc_ld(int in_features) { return (in_features + 1) | 1; }
static inline int zce_classes_per_workgroup(int in_features) {
  const int c = ZCE_LDS_FLOATS / zce_acc_ld(in_features);
  return c > ZCE_MAX_CLASSES ? ZCE_MAX_CLASSES : c;
}
// slabs of rows for the uniform sums: at most 1024, at least 64 rows each
static void zce_esum_plan(int64_t rows, int* slabs, int64_t* rows_per_slab) {
  int64_t want = (rows + 63) / 64;
  if (want > 1024) want = 1024;
  if (want < 1) want = 1;
  const int64_t rps = (rows + want - 1) / want;
  *rows_per_slab = rps;
  *slabs = (int)((rows + rps - 1) / rps);
}

extern "C" int pdnz_cross_entropy_fwd_f32(const float* logits, const int64_t* targets, int masked, int64_t ignore_index,
                                          int64_t rows, int V, int reduction, float label_smoothing, float z_loss,
                                          float* loss_row, float* lse_row, float* loss_out, float* stats, int* err_flag,
                                          void* stream) {
  PDN_CHECK_ARG(rows > 0 && V > 0 && reduction >= 0 && reduction <= 2, "pdnz_cross_entropy_fwd_f32: empty input or bad reduction");
  PDN_CHECK_ARG(logits && targets && loss_row && lse_row && err_flag && (reduction == 0 || (loss_out && stats)),
                "pdnz_cross_entropy_fwd_f32: null operand");
  pdn_count(PDN_CNT_SMOOTH_LOSS);
  hipStream_t st = (hipStream_t)stream;
  if (zce_reg_row_ok(V, logits, logits)) {
    hipLaunchKernelGGL(zce_fwd_reg_kernel, dim3(zce_reg_grid(rows)), dim3(1024), 0, st, logits, targets, masked, ignore_index,
                       loss_row, lse_row, rows, V, label_smoothing, z_loss, err_flag);
  } else {
    // long rows: few, fat workgroups; short ones: a wave is enough
    const int threads = V >= 4096 ? 1024 : (V > 256 ? 256 : 64);
    const int g = (int)(V >= 4096 ? (rows < 512 ? rows : 512) : (rows < 65535 ? rows : 65535));
    hipLaunchKernelGGL(zce_fwd_rows_kernel, dim3(g), dim3(threads), 0, st, logits, targets, masked, ignore_index, loss_row, lse_row,
                       rows, V, label_smoothing, z_loss, err_flag);
  }
  PDN_LAUNCH_CHECK();
  if (reduction != 0) {
    hipLaunchKernelGGL(zce_reduce_kernel, dim3(1), dim3(1024), 0, st, targets, masked, ignore_index, (const float*)loss_row, rows,
                       reduction == 2 ? 1 : 0, stats, loss_out);
    PDN_LAUNCH_CHECK();
  }
  return PDN_OK;
}

extern "C" int pdnz_cross_entropy_bwd_f32(const float* logits, const int64_t* targets, int masked, int64_t ignore_index,
                                          const float* lse_row, const float* u, const float* upstream, const float* stats,
                                          float label_smoothing, float z_loss, float* dlogits, int64_t rows, int V,
                                          void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && targets && lse_row && dlogits && V > 0 && rows > 0, "pdnz_cross_entropy_bwd_f32: bad arguments");
  pdn_count(PDN_CNT_SMOOTH_LOSS);
  hipStream_t st = (hipStream_t)stream;
  if (zce_reg_row_ok(V, logits, dlogits)) {
    hipLaunchKernelGGL(zce_bwd_reg_kernel, dim3(zce_reg_grid(rows)), dim3(1024), 0, st, logits, targets, masked, ignore_index,
                       lse_row, u, upstream, stats, label_smoothing, z_loss, dlogits, rows, V);
  } else {
    const int g = (int)(rows < 65535 ? rows : 65535);
    hipLaunchKernelGGL(zce_bwd_rows_kernel, dim3(g), dim3(V > 256 ? 256 : 64), 0, st, logits, targets, masked, ignore_index,
                       lse_row, u, upstream, stats, label_smoothing, z_loss, dlogits, rows, V);
  }
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnz_weight_sums_f32(const float* W, const float* bias, int in_features, int V, float* wsum, void* stream) {
  PDN_CHECK_ARG(W && wsum && in_features > 0 && V > 0, "pdnz_weight_sums_f32: bad arguments");
  pdn_count(PDN_CNT_SMOOTH_LOSS);
  hipLaunchKernelGGL(zce_weight_sums_kernel, dim3(in_features + 1), dim3(256), 0, (hipStream_t)stream, W, bias, in_features, V,
                     wsum);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnz_linear_ce_finish_f32(const float* logits, int64_t ldl, float* lse, const int64_t* targets, int masked,
                                         int64_t ignore_index, const float* x, int64_t ldx, const float* wsum, int64_t rows,
                                         int V, int in_features, int reduction, float label_smoothing, float z_loss,
                                         float* loss_row, float* loss_out, float* stats, int64_t* targets_safe, int* err_flag,
                                         void* stream) {
  PDN_CHECK_ARG(rows > 0 && V > 0 && ldl >= V && reduction >= 0 && reduction <= 2,
                "pdnz_linear_ce_finish_f32: empty input or bad reduction");
  PDN_CHECK_ARG(logits && lse && targets && loss_row && targets_safe && err_flag && (reduction == 0 || (loss_out && stats)),
                "pdnz_linear_ce_finish_f32: null operand");
  PDN_CHECK_ARG(label_smoothing == 0.f || (x && wsum && in_features > 0 && ldx >= in_features),
                "pdnz_linear_ce_finish_f32: label smoothing needs x and wsum");
  pdn_count(PDN_CNT_SMOOTH_LOSS);
  hipStream_t st = (hipStream_t)stream;
  const int64_t blocks = (rows + 3) / 4;
  hipLaunchKernelGGL(zce_finish_rows_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, st, logits, ldl, lse,
                     targets, masked, ignore_index, x, ldx, wsum, rows, V, in_features, label_smoothing, z_loss, loss_row,
                     targets_safe, err_flag);
  PDN_LAUNCH_CHECK();
  if (reduction != 0) {
    hipLaunchKernelGGL(zce_reduce_kernel, dim3(1), dim3(1024), 0, st, (const int64_t*)targets_safe, 1, (int64_t)V,
                       (const float*)loss_row, rows, reduction == 2 ? 1 : 0, stats, loss_out);
    PDN_LAUNCH_CHECK();
  }
  return PDN_OK;
}

extern "C" int pdnz_row_coefficients_f32(const float* lse_masked, const int64_t* targets_safe, const float* u,
                                         const float* upstream, const float* stats, float label_smoothing, float z_loss,
                                         int64_t rows, int V, float* u_out, float* c_out, float* e_out, void* stream) {
  if (rows == 0) return PDN_OK;
  PDN_CHECK_ARG(lse_masked && targets_safe && u_out && c_out && e_out && rows > 0 && V > 0,
                "pdnz_row_coefficients_f32: bad arguments");
  pdn_count(PDN_CNT_SMOOTH_LOSS);
  hipLaunchKernelGGL(zce_coefficients_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, lse_masked,
                     targets_safe, u, upstream, stats, label_smoothing, z_loss, rows, V, u_out, c_out, e_out);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int64_t pdnz_linear_ce_corrections_workspace_bytes(int64_t rows, int V, int in_features) {
  if (rows <= 0 || V <= 0 || in_features <= 0) return 0;
  int slabs;
  int64_t rps;
  zce_esum_plan(rows, &slabs, &rps);
  return (int64_t)(slabs + 1) * (in_features + 1) * 4;
}

extern "C" int pdnz_linear_ce_corrections_f32(const float* x, int64_t ldx, const float* W, const float* wsum,
                                              const int64_t* targets_safe, const float* c, const float* e, float* dx, float* dW,
                                              float* dbias, int64_t rows, int V, int in_features, void* workspace,
                                              int64_t workspace_bytes, void* stream) {
  if (rows == 0 || V == 0) return PDN_OK;
  PDN_CHECK_ARG(x && W && targets_safe && c && rows > 0 && V > 0 && in_features > 0 && ldx >= in_features,
                "pdnz_linear_ce_corrections_f32: bad arguments");
  PDN_CHECK_ARG(!e || wsum, "pdnz_linear_ce_corrections_f32: the uniform term needs wsum");
  const int cpw = zce_classes_per_workgroup(in_features);
  if (cpw < 1) {
    pdn_set_error("pdnz_linear_ce_corrections_f32: in_features %d above %d", in_features, ZCE_LDS_FLOATS - 2);
    return PDN_EUNSUPPORTED;
  }
  pdn_count(PDN_CNT_SMOOTH_LOSS);
  hipStream_t st = (hipStream_t)stream;
  if (dx) {
    hipLaunchKernelGGL(zce_dx_kernel, dim3(zce_stream_grid(rows * in_features)), dim3(256), 0, st, dx, W, wsum, targets_safe, c, e,
                       rows, V, in_features);
    PDN_LAUNCH_CHECK();
  }
  if (!dW && !dbias) return PDN_OK;
  float* r = nullptr;
  if (e) {
    if (!workspace || workspace_bytes < pdnz_linear_ce_corrections_workspace_bytes(rows, V, in_features)) {
      pdn_set_error("pdnz_linear_ce_corrections_f32: workspace too small");
      return PDN_EWORKSPACE;
    }
    int slabs;
    int64_t rps;
    zce_esum_plan(rows, &slabs, &rps);
    float* part = (float*)workspace;
    r = part + (int64_t)slabs * (in_features + 1);
    const unsigned kb = (unsigned)((in_features + 1 + 255) / 256);
    hipLaunchKernelGGL(zce_esum_part_kernel, dim3(kb, (unsigned)slabs), dim3(256), 0, st, x, ldx, e, rows, in_features, rps, part);
    PDN_LAUNCH_CHECK();
    hipLaunchKernelGGL(zce_esum_reduce_kernel, dim3(kb), dim3(256), 0, st, (const float*)part, slabs, in_features, r);
    PDN_LAUNCH_CHECK();
  }
  const int ld = zce_acc_ld(in_features);
  hipLaunchKernelGGL(zce_class_sums_kernel, dim3((unsigned)((V + cpw - 1) / cpw)), dim3(256), (size_t)cpw * ld * sizeof(float), st, x,
                     ldx, targets_safe, c, (const float*)r, dW, dbias, rows, V, in_features, cpw, ld);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
