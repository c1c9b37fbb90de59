// The passes over x of the split-fp16 TN pipeline (csrc/lm_head_dw_split.hip, csrc/outres_tn_split.hip; gfx950 only):
//
//   x[:, d] 2^s(d) = xh + xl / 2048      one power of two per COLUMN d of x = per row of dW
//
// in three launches: partial column maxima over ranges of rows, the exponent of every column, then the plane images, one per
// piece of 32 tokens, transposed, in LDS order (csrc/split_tn_index.h).  With lse and targets the images are 37 KiB and
// their tails carry the row statistics of the NEXT piece (the lm_head weight gradient), without 36 KiB.  Where x is the output
// of an RMSNorm that was never written, ONE launch forms it from the rows before the norm and takes the exponents from the
// norm weight (stn_split_xn_kernel below).
#include "split_tn.h"

#define STN_L2E 1.4426950408889634f

// ---- column maxima over a range of rows (partial), then the exponent of every column ---------------------------------
// 288 threads: thread (c4 = tid % 72, g = tid / 72) takes the float4 c4 of rows g, g + 4, .. of the block's range
__global__ __launch_bounds__(288) void stn_x_colmax_kernel(const float* __restrict__ x, int64_t ldx, int rows, int rows_per_block,
                                                            float* __restrict__ partial) {
  __shared__ float sm[4][STN_N];
  const int c4 = threadIdx.x % 72, g = threadIdx.x / 72;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 z = m;                 // fmaxf drops a NaN: 0 * v stays 0 for every finite v and turns NaN for Inf and NaN
#pragma unroll 4
  for (int r = r0 + g; r < r1; r += 4) {
    const float4 v = *reinterpret_cast<const float4*>(x + (int64_t)r * ldx + 4 * c4);
    m.x = fmaxf(m.x, fabsf(v.x)); m.y = fmaxf(m.y, fabsf(v.y)); m.z = fmaxf(m.z, fabsf(v.z)); m.w = fmaxf(m.w, fabsf(v.w));
    z.x = fmaf(v.x, 0.f, z.x); z.y = fmaf(v.y, 0.f, z.y); z.z = fmaf(v.z, 0.f, z.z); z.w = fmaf(v.w, 0.f, z.w);
  }
  if (z.x != z.x) m.x = INFINITY;
  if (z.y != z.y) m.y = INFINITY;
  if (z.z != z.z) m.z = INFINITY;
  if (z.w != z.w) m.w = INFINITY;
  sm[g][4 * c4 + 0] = m.x; sm[g][4 * c4 + 1] = m.y; sm[g][4 * c4 + 2] = m.z; sm[g][4 * c4 + 3] = m.w;
  __syncthreads();
  const int d = threadIdx.x;
  partial[(int64_t)blockIdx.x * STN_N + d] = fmaxf(fmaxf(sm[0][d], sm[1][d]), fmaxf(sm[2][d], sm[3][d]));
}

// one workgroup per column: thread i takes parts i, i + 256, .. (eight trips at 2048 parts over 288 workgroups; nine
// workgroups of 32 columns x 8 part groups made 256 dependent trips, 51 us of latency)
__global__ __launch_bounds__(256) void stn_x_shift_kernel(const float* __restrict__ partial, int nparts, int* __restrict__ xsh) {
  __shared__ float sm[4];
  const int d = blockIdx.x;
  float m = 0.f;
  for (int b = threadIdx.x; b < nparts; b += 256) m = fmaxf(m, partial[(int64_t)b * STN_N + d]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) xsh[d] = ls_shift(fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])));
}

// ---- the plane images, one workgroup per piece of 32 tokens; TAIL: the row statistics of the NEXT piece behind the planes --
template <int XKIB, bool TAIL>
__device__ __forceinline__ void stn_split_x(const float* __restrict__ x, int64_t ldx, const int* __restrict__ xsh,
                                            const float* __restrict__ lse, const int64_t* __restrict__ targets, int rows,
                                            char* __restrict__ ximg) {
  __shared__ __attribute__((aligned(16))) float raw[STN_KP * STN_N];
  char* img = ximg + (int64_t)blockIdx.x * stn_xpiece(XKIB);
  const float* xp = x + (int64_t)blockIdx.x * STN_KP * ldx;
  // the piece by 16-byte loads, all nine of a thread in flight, staged raw in LDS (the chunks of a row rotated per quarter)
  float4 v[STN_PASS_LOADS];
#pragma unroll
  for (int e = 0; e < STN_PASS_LOADS; ++e) {
    const int i = threadIdx.x + STN_PASS_THREADS * e;
    v[e] = *reinterpret_cast<const float4*>(xp + (int64_t)stn_pass_row(i) * ldx + 4 * stn_pass_chunk(i));
  }
#pragma unroll
  for (int e = 0; e < STN_PASS_LOADS; ++e) {
    const int i = threadIdx.x + STN_PASS_THREADS * e;
    *reinterpret_cast<float4*>(raw + stn_pass_lds(stn_pass_row(i), 4 * stn_pass_chunk(i))) = v[e];
  }
  __syncthreads();
  // the units in image order: a wave's store instruction is 1 KiB of whole lines in either plane
#pragma unroll
  for (int e = 0; e < (STN_N * 4 + STN_PASS_THREADS - 1) / STN_PASS_THREADS; ++e) {
    const int u = threadIdx.x + STN_PASS_THREADS * e;
    if (u < STN_N * 4) {
      const int d = stn_pass_unit_d(u), q = stn_pass_unit_q(u);
      const int sh = xsh[d];
      f16x8 hv, lv;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        _Float16 h, l;
        ls_split(raw[stn_pass_lds(8 * q + k, d)], sh, h, l);
        hv[k] = h; lv[k] = l;
      }
      *reinterpret_cast<f16x8*>(img + 16 * u) = hv;
      *reinterpret_cast<f16x8*>(img + STN_PLANE + 16 * u) = lv;
    }
  }
  // tail: 1 KiB = 256 dwords; dwords 0..31 -lse log2 e, 32..63 the targets, the rest zero
  if (TAIL) {
    const int i = threadIdx.x;
    const int64_t t = ((int64_t)blockIdx.x + 1) * STN_KP + (i & 31);
    unsigned v = 0u;
    if (i < 64 && t < rows) v = i < 32 ? __float_as_uint(-STN_L2E * lse[t]) : (unsigned)(int)targets[t];
    reinterpret_cast<unsigned*>(img + LDW_TAIL)[i] = v;
  }
}
// (two kernels of their own arguments around the one body: neither carries what it does not read)
__global__ __launch_bounds__(256) void stn_split_x_kernel(const float* __restrict__ x, int64_t ldx, const int* __restrict__ xsh,
                                                           char* __restrict__ ximg) {
  stn_split_x<OTS_XKIB, false>(x, ldx, xsh, nullptr, nullptr, 0, ximg);
}
__global__ __launch_bounds__(256) void stn_split_x_tail_kernel(const float* __restrict__ x, int64_t ldx, const int* __restrict__ xsh,
                                                                const float* __restrict__ lse, const int64_t* __restrict__ targets,
                                                                int rows, char* __restrict__ ximg) {
  stn_split_x<LDW_XKIB, true>(x, ldx, xsh, lse, targets, rows, ximg);
}

// ---- the plane images of an RMSNorm OUTPUT that is never written: xn[t][d] = x[t][d] * (1 / rms[t]) * w[d], formed here with
// the arithmetic of the projection kernels (csrc/rowtile_split.hip, csrc/gemm_rowtile.hip), in ONE launch.  No pass for the
// column maxima: with rms[t] >= sqrt(mean_d x[t][d]^2) every |x[t][d]| <= sqrt(288) rms[t], so |xn[t][d]| < 17 |w[d]| and
// the exponent of column d follows from w[d] alone (ls_shift puts the BOUND into [2^8, 2^9); a zero or non-finite w[d]: 0).
// The same loads, staging and image as stn_split_x; workgroup 0 leaves the 288 exponents for the main kernel's drain.
__global__ __launch_bounds__(256) void stn_split_xn_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                            const float* __restrict__ rms, int* __restrict__ xsh,
                                                            char* __restrict__ ximg) {
  __shared__ __attribute__((aligned(16))) float raw[STN_KP * STN_N];
  __shared__ float inv[STN_KP];
  char* img = ximg + (int64_t)blockIdx.x * stn_xpiece(OTS_XKIB);
  const float* xp = x + (int64_t)blockIdx.x * STN_KP * ldx;
  float4 v[STN_PASS_LOADS];
#pragma unroll
  for (int e = 0; e < STN_PASS_LOADS; ++e) {
    const int i = threadIdx.x + STN_PASS_THREADS * e;
    v[e] = *reinterpret_cast<const float4*>(xp + (int64_t)stn_pass_row(i) * ldx + 4 * stn_pass_chunk(i));
  }
  if (threadIdx.x < STN_KP) inv[threadIdx.x] = 1.f / rms[(int64_t)blockIdx.x * STN_KP + threadIdx.x];
  if (blockIdx.x == 0)
    for (int d = threadIdx.x; d < STN_N; d += STN_PASS_THREADS) xsh[d] = ls_shift(17.f * fabsf(w[d]));
#pragma unroll
  for (int e = 0; e < STN_PASS_LOADS; ++e) {
    const int i = threadIdx.x + STN_PASS_THREADS * e;
    *reinterpret_cast<float4*>(raw + stn_pass_lds(stn_pass_row(i), 4 * stn_pass_chunk(i))) = v[e];
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < (STN_N * 4 + STN_PASS_THREADS - 1) / STN_PASS_THREADS; ++e) {
    const int u = threadIdx.x + STN_PASS_THREADS * e;
    if (u < STN_N * 4) {
      const int d = stn_pass_unit_d(u), q = stn_pass_unit_q(u);
      const float wd = w[d];
      const int sh = ls_shift(17.f * fabsf(wd));
      f16x8 hv, lv;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        _Float16 h, l;
        ls_split(raw[stn_pass_lds(8 * q + k, d)] * inv[8 * q + k] * wd, sh, h, l);
        hv[k] = h; lv[k] = l;
      }
      *reinterpret_cast<f16x8*>(img + 16 * u) = hv;
      *reinterpret_cast<f16x8*>(img + STN_PLANE + 16 * u) = lv;
    }
  }
}

int* stn_xn_planes_launch(const float* x, int64_t ldx, const float* w, const float* rms, int rows, void* extra, void* stream) {
  const int npieces = rows / STN_KP;
  char* ximg = static_cast<char*>(extra);
  int* xsh = reinterpret_cast<int*>(ximg + (int64_t)npieces * stn_xpiece(OTS_XKIB));
  hipLaunchKernelGGL(stn_split_xn_kernel, dim3(npieces), dim3(256), 0, (hipStream_t)stream, x, ldx, w, rms, xsh, ximg);
  return xsh;
}

int* stn_x_planes_launch(const float* x, int64_t ldx, int rows, void* extra, const float* lse, const int64_t* targets, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool tail = lse != nullptr;
  const int npieces = rows / STN_KP;
  char* ximg = static_cast<char*>(extra);
  int* xsh = reinterpret_cast<int*>(ximg + (int64_t)npieces * stn_xpiece(tail ? LDW_XKIB : OTS_XKIB));
  float* partial = reinterpret_cast<float*>(ximg);               // parked in the image region until the plane pass
  const int nparts = stn_partials(rows);
  const int rpb = (rows + nparts - 1) / nparts;
  const int nblk = (rows + rpb - 1) / rpb;
  hipLaunchKernelGGL(stn_x_colmax_kernel, dim3(nblk), dim3(288), 0, st, x, ldx, rows, rpb, partial);
  hipLaunchKernelGGL(stn_x_shift_kernel, dim3(STN_N), dim3(256), 0, st, partial, nblk, xsh);
  if (tail) hipLaunchKernelGGL(stn_split_x_tail_kernel, dim3(npieces), dim3(256), 0, st, x, ldx, xsh, lse, targets, rows, ximg);
  else hipLaunchKernelGGL(stn_split_x_kernel, dim3(npieces), dim3(256), 0, st, x, ldx, xsh, ximg);
  return xsh;
}
