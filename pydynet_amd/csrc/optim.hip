// Optimizer-step extensions (gfx950): global-norm gradient clipping, decoupled weight decay and the device-side
// control words that let both run inside a replayed hipGraph.  They extend the multi-tensor Adam of csrc/fused.hip
// (optim/optimizer.py:185-196 of the reference, which has no counterpart for any of this); the NumPy statement of
// the arithmetic is pydynet_amd/optim/clip.py.  Entry points: include/pdn_optim.h (prefix pdnx_).
//
//   table   : device int64[nchunks][5] = {p, g, m, v (addresses), n (elements in chunk)} -- Adam's chunk table
//   partials: device double[nchunks], one sum of squares per chunk
//   ctl     : device float[4] = {norm, coef, skip (0 or 1), skipped steps so far}
//
//   norm = |grad_scale| * sqrt(sum g^2)     coef = min(1, max_norm / (norm + 1e-6))     (max_norm <= 0: coef 1)
//   norm not finite: coef 0, skip 1 -- the update kernel returns before it touches p, m or v
//
// Everything is reduced in a fixed order (no atomics): the same gradients give the same bits.
#include "common.h"
#include <math.h>

#define SQ4(A, V) A += (double)V.x * (double)V.x + (double)V.y * (double)V.y + (double)V.z * (double)V.z + (double)V.w * (double)V.w;

// One workgroup per chunk, column 1 (g) and 4 (n) of the table only.  A float squared is exact in double and a chunk
// holds 2^14 of them, so a chunk's partial is the exact sum rounded a few times at 2^-53: only the final cast to
// float32 is visible.  The kernel reads 4 B per parameter and writes 8 B per chunk; the fp64 FMAs hide behind HBM.
__global__ void __launch_bounds__(256) grad_sqnorm_multi_kernel(const int64_t* __restrict__ table,
                                                                double* __restrict__ partials) {
  __shared__ double red[16];
  const int64_t* e = table + (int64_t)blockIdx.x * 5;
  const float* g = (const float*)e[1];
  const int n = (int)e[4];
  const int n4 = (e[1] & 15) == 0 ? n >> 2 : 0;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int i = threadIdx.x;
  for (; i + 3 * 256 < n4; i += 4 * 256) {             // four independent 16 B loads in flight per lane
    const float4 v0 = g4[i], v1 = g4[i + 256], v2 = g4[i + 512], v3 = g4[i + 768];
    SQ4(a0, v0) SQ4(a1, v1) SQ4(a2, v2) SQ4(a3, v3)
  }
  for (; i < n4; i += 256) {
    const float4 v0 = g4[i];
    SQ4(a0, v0)
  }
  for (int j = n4 * 4 + threadIdx.x; j < n; j += 256) {
    const double x = (double)g[j];
    a1 += x * x;
  }
  const double s = block_sum((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// One workgroup: thread t adds partials[t], partials[t + 256], ... in that order, then the block reduction.
// `state` non-null (replayed step): this launch is also the step's tick (adam_tick_kernel of csrc/fused.hip):
// state = {t, lr} doubles -> step_dev = {lr * sqrt(1-b2^t)/(1-b1^t), lr * wd}, t += 1.  The tick runs whether
// or not the update is skipped, so eager and replayed steps count alike.  `ctl` null: the tick alone.
__global__ void __launch_bounds__(256) grad_norm_finalize_kernel(const double* __restrict__ partials, int nchunks,
                                                                 float grad_scale, float max_norm, float* __restrict__ ctl,
                                                                 double* __restrict__ state, float* __restrict__ step_dev,
                                                                 double b1, double b2, double wd) {
  __shared__ double red[16];
  if (ctl) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += 256) s += partials[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
      const double norm = fabs((double)grad_scale) * sqrt(s);
      const bool finite = isfinite(norm);
      double coef = 1.0;
      if (max_norm > 0.f) coef = fmin(1.0, (double)max_norm / (norm + 1e-6));
      if (!finite) coef = 0.0;
      ctl[0] = (float)norm;
      ctl[1] = (float)coef;
      ctl[2] = finite ? 0.f : 1.f;
      ctl[3] += finite ? 0.f : 1.f;
    }
  }
  if (state && threadIdx.x == 0) {
    const double t = state[0], lr = state[1];
    step_dev[0] = (float)(lr * sqrt(1.0 - pow(b2, t)) / (1.0 - pow(b1, t)));
    step_dev[1] = (float)(lr * wd);
    state[0] = t + 1.0;
  }
}

// adam_multi_kernel's loop (csrc/fused.hip) with the clip coefficient and the decoupled decay:
//   ctl non-null: return when ctl[2] != 0 (uniform over the grid), else grad_scale *= ctl[1]
//   DECOUPLED:    p -= lr_wd * p first, and no wd * p in the gradient
// step_dev non-null (replayed step): {step, lr_wd} are read there.  28 B per parameter, as Adam.
template <bool DECOUPLED>
__global__ void __launch_bounds__(256) adam_multi_clip_kernel(const int64_t* __restrict__ table, float step, float lr_wd,
                                                              float b1, float b2, float one_m_b1, float one_m_b2, float eps,
                                                              float wd, float grad_scale, const float* __restrict__ ctl,
                                                              const float* __restrict__ step_dev) {
  if (ctl) {
    if (ctl[2] != 0.f) return;
    grad_scale *= ctl[1];
  }
  if (step_dev) { step = step_dev[0]; lr_wd = step_dev[1]; }
  const int64_t* e = table + (int64_t)blockIdx.x * 5;
  float* p = (float*)e[0]; const float* g = (const float*)e[1];
  float* m = (float*)e[2]; float* v = (float*)e[3];
  const int n = (int)e[4];
  const bool al = ((e[0] | e[1] | e[2] | e[3]) & 15) == 0;
  const int n4 = al ? n >> 2 : 0;
#define ADAMC1(P, G, M, V)                                \
  {                                                       \
    float gg;                                             \
    if (DECOUPLED) { P -= lr_wd * P; gg = G * grad_scale; } \
    else gg = G * grad_scale + wd * P;                    \
    M = M * b1 + one_m_b1 * gg;                           \
    V = V * b2 + one_m_b2 * (gg * gg);                    \
    P -= step * M / (sqrtf(V) + eps);                     \
  }
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv0 = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    ADAMC1(pv.x, gv0.x, mv.x, vv.x) ADAMC1(pv.y, gv0.y, mv.y, vv.y)
    ADAMC1(pv.z, gv0.z, mv.z, vv.z) ADAMC1(pv.w, gv0.w, mv.w, vv.w)
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (int i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) {
    float P = p[i], M = m[i], V = v[i];
    const float G = g[i];
    ADAMC1(P, G, M, V)
    p[i] = P; m[i] = M; v[i] = V;
  }
}

// g *= ctl[1] for optimizers that do not take the coefficient themselves (nn.utils.clip_grad_norm_).  Nothing is
// written when the step is skipped (ctl[2] != 0) or when nothing is clipped (g * 1 is g).
__global__ void __launch_bounds__(256) grad_scale_multi_kernel(const int64_t* __restrict__ table,
                                                               const float* __restrict__ ctl) {
  const float c = ctl[1];
  if (ctl[2] != 0.f || c == 1.f) return;
  const int64_t* e = table + (int64_t)blockIdx.x * 5;
  float* g = (float*)e[1];
  const int n = (int)e[4];
  const int n4 = (e[1] & 15) == 0 ? n >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += 256) {
    float4 x = reinterpret_cast<float4*>(g)[i];
    x.x *= c; x.y *= c; x.z *= c; x.w *= c;
    reinterpret_cast<float4*>(g)[i] = x;
  }
  for (int i = n4 * 4 + threadIdx.x; i < n; i += 256) g[i] *= c;
}

// The ABI carries the betas as float32: 0.999 arrives as 0.99900001287, and 1 - that misses 0.001 by 1.3e-5 of its value,
// which v and a_t would inherit (pdn_adam_multi_f32 is handed 1 - beta by the host for this reason).  So beta is rounded to
// seven decimals first.  That is a guess at what the caller wrote: exact for betas of seven decimals or fewer; a beta
// with more digits is ALTERED, by up to 5e-8 (floats in [0.5, 1) are 6e-8 apart, so by less than one ulp of what was
// passed).  adam_tick_kernel's path (csrc/fused.hip) does not do this: it uses (double)beta and 1.f - beta.
static double beta_decimal(float b) { return nearbyint((double)b * 1e7) / 1e7; }

static int launch_norm(const int64_t* table, int nchunks, float grad_scale, float max_norm, double* partials, float* ctl,
                       double* state, float* step_dev, float b1, float b2, float wd, hipStream_t st) {
  hipLaunchKernelGGL(grad_sqnorm_multi_kernel, dim3(nchunks), dim3(256), 0, st, table, partials);
  PDN_LAUNCH_CHECK();
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, nchunks, grad_scale,
                     max_norm, ctl, state, step_dev, beta_decimal(b1), beta_decimal(b2), (double)wd);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

static int launch_update(const int64_t* table, int nchunks, float step, float lr_wd, float b1, float b2, float eps, float wd,
                         float grad_scale, int decoupled, const float* ctl, const float* step_dev, hipStream_t st) {
  const float one_m_b1 = (float)(1.0 - beta_decimal(b1)), one_m_b2 = (float)(1.0 - beta_decimal(b2));
  if (decoupled)
    hipLaunchKernelGGL(adam_multi_clip_kernel<true>, dim3(nchunks), dim3(256), 0, st, table, step, lr_wd, b1, b2, one_m_b1,
                       one_m_b2, eps, wd, grad_scale, ctl, step_dev);
  else
    hipLaunchKernelGGL(adam_multi_clip_kernel<false>, dim3(nchunks), dim3(256), 0, st, table, step, lr_wd, b1, b2, one_m_b1,
                       one_m_b2, eps, wd, grad_scale, ctl, step_dev);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnx_grad_norm_multi_f32(const int64_t* chunk_table_dev, int nchunks, float grad_scale, float max_norm,
                                       double* partials_dev, float* ctl_dev, void* stream) {
  if (nchunks == 0) return PDN_OK;
  PDN_CHECK_ARG(chunk_table_dev && nchunks > 0 && partials_dev && ctl_dev, "pdnx_grad_norm_multi_f32: bad arguments");
  return launch_norm(chunk_table_dev, nchunks, grad_scale, max_norm, partials_dev, ctl_dev, nullptr, nullptr, 0.f, 0.f, 0.f,
                     (hipStream_t)stream);
}

extern "C" int pdnx_grad_scale_multi_f32(const int64_t* chunk_table_dev, int nchunks, const float* ctl_dev, void* stream) {
  if (nchunks == 0) return PDN_OK;
  PDN_CHECK_ARG(chunk_table_dev && nchunks > 0 && ctl_dev, "pdnx_grad_scale_multi_f32: bad arguments");
  hipLaunchKernelGGL(grad_scale_multi_kernel, dim3(nchunks), dim3(256), 0, (hipStream_t)stream, chunk_table_dev, ctl_dev);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

extern "C" int pdnx_adam_multi_clip_f32(const int64_t* chunk_table_dev, int nchunks, float step, float lr_wd, float beta1,
                                       float beta2, float eps, float weight_decay, float grad_scale, int decoupled,
                                       const float* ctl_dev, void* stream) {
  if (nchunks == 0) return PDN_OK;
  PDN_CHECK_ARG(chunk_table_dev && nchunks > 0, "pdnx_adam_multi_clip_f32: bad arguments");
  return launch_update(chunk_table_dev, nchunks, step, lr_wd, beta1, beta2, eps, weight_decay, grad_scale, decoupled, ctl_dev,
                       nullptr, (hipStream_t)stream);
}

extern "C" int pdnx_adam_multi_clip_tick_f32(const int64_t* chunk_table_dev, int nchunks, double* state_dev, float* step_dev,
                                            float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                            float max_norm, int decoupled, double* partials_dev, float* ctl_dev, void* stream) {
  PDN_CHECK_ARG(state_dev && step_dev, "pdnx_adam_multi_clip_tick_f32: null state");
  PDN_CHECK_ARG(nchunks >= 0 && (nchunks == 0 || chunk_table_dev), "pdnx_adam_multi_clip_tick_f32: bad arguments");
  PDN_CHECK_ARG(!ctl_dev || nchunks == 0 || partials_dev, "pdnx_adam_multi_clip_tick_f32: ctl without partials");
  hipStream_t st = (hipStream_t)stream;
  if (ctl_dev && nchunks > 0) {                          // partials, finalize + tick, update
    const int rc = launch_norm(chunk_table_dev, nchunks, grad_scale, max_norm, partials_dev, ctl_dev, state_dev, step_dev,
                               beta1, beta2, weight_decay, st);
    if (rc) return rc;
  } else {                                               // no clipping (decoupled decay alone): the tick alone
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)nullptr, 0, 1.f, 0.f,
                       (float*)nullptr, state_dev, step_dev, beta_decimal(beta1), beta_decimal(beta2), (double)weight_decay);
    PDN_LAUNCH_CHECK();
  }
  if (nchunks == 0) return PDN_OK;
  return launch_update(chunk_table_dev, nchunks, 0.f, 0.f, beta1, beta2, eps, weight_decay, grad_scale, decoupled, ctl_dev,
                       step_dev, st);
}
