// Prefix caching (Llama.serve(prefix_cache=...), statement: pydynet_amd/llm/prefix.py): a row admitted with a prompt
// whose leading tokens another cache row already holds takes that row's keys and values instead of computing them.
//   kv_copy_prefix_kernel   copy i: positions [0, len[i]) of row src[i] go to row dst[i], for every cache tensor, in
//                           one launch, each source read as it was before the launch.
#include "common.h"

#include <algorithm>

#define KCP_MAX 256                // copies per launch
#define KCP_THREADS 256
typedef float kcp_f4 __attribute__((ext_vector_type(4)));

// grid (column slices, position groups, n_tensors), 256 threads.  A copy only ever moves position t of one row to position
// t of another, so the hazard (row 2 <- row 5 while row 5 <- row 2; chains 1 <- 2 <- 3) is per position: a workgroup owns
// (tensor, column slice, the TP positions of a group) for ALL rows -- the scheme of kv_reorder_kernel (csrc/beam.hip).
// It loads every copy's source there into registers, waits, then stores; no other workgroup touches those bytes, so
// every source is read as it was before the launch.  An item is (copy i, position t0 + tp, column c) with
// n_copies * TP <= 256 (copy, position) pairs and CW columns of type T per slice: 256 * K / CW = 256 pairs, K registers
// of T per thread.  T = 4 floats (CW 8, K 8: 128 contiguous bytes per row and position) when D and the row stride are
// multiples of 4, else float (CW 16, K 16).
template <typename T, int CW, int K>
__global__ __launch_bounds__(KCP_THREADS) void kv_copy_prefix_kernel(float* const* __restrict__ caches, int64_t bs,
                                                                     int n_rows, int max_len, int D,
                                                                     const int* __restrict__ dst,
                                                                     const int* __restrict__ src,
                                                                     const int* __restrict__ len, int n, int TP) {
  constexpr int E = sizeof(T) / 4;               // floats per element
  constexpr int PL = KCP_THREADS / CW;           // (copy, position) pairs per pass over the threads
  static_assert(PL * K == KCP_MAX, "256 pairs per workgroup");
  __shared__ int s_dst[KCP_MAX], s_src[KCP_MAX], s_len[KCP_MAX];
  __shared__ int s_pi[KCP_MAX], s_pt[KCP_MAX];   // pair -> (copy, position within the group); copy -1: no such pair
  __shared__ int s_tmax;
  const int tid = threadIdx.x;
  if (tid == 0) s_tmax = 0;
  __syncthreads();
  if (tid < n) {
    const int d = dst[tid], s = src[tid], l = len[tid];
    const bool ok = d != s && d >= 0 && d < n_rows && s >= 0 && s < n_rows && l > 0;
    const int m = ok ? min(l, max_len) : 0;
    s_dst[tid] = ok ? d : 0;
    s_src[tid] = ok ? s : 0;
    s_len[tid] = m;
    if (m > 0) atomicMax(&s_tmax, m);
  }
  {
    const int tp = tid / n;
    s_pi[tid] = tp < TP ? tid - tp * n : -1;
    s_pt[tid] = tp;
  }
  __syncthreads();
  const int tmax = s_tmax;
  float* base = caches[blockIdx.z];
  const int c0 = blockIdx.x * CW, c = tid % CW, pb = tid / CW;
  const bool col = c0 + c < D / E;
  const int64_t coff = (int64_t)E * (c0 + c);
  for (int t0 = blockIdx.y * TP; t0 < tmax; t0 += gridDim.y * TP) {
    T v[K];
    unsigned live = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = s_pi[pb + k * PL], t = t0 + s_pt[pb + k * PL];
      v[k] = T(0);
      if (col && i >= 0 && t < s_len[i]) {
        v[k] = *reinterpret_cast<const T*>(base + (int64_t)s_src[i] * bs + (int64_t)t * D + coff);
        live |= 1u << k;
      }
    }
    __syncthreads();                              // (every source of these positions is loaded before any store)
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (live >> k & 1) {
        const int i = s_pi[pb + k * PL], t = t0 + s_pt[pb + k * PL];
        *reinterpret_cast<T*>(base + (int64_t)s_dst[i] * bs + (int64_t)t * D + coff) = v[k];
      }
    }
  }
}

extern "C" int pdn_kv_copy_prefix_rows_f32(float* const* caches, int n_tensors, int64_t batch_stride, int n_rows,
                                           int max_len, int D, const int* dst, const int* src, const int* len,
                                           int n_copies, void* stream) {
  if (n_tensors == 0 || n_copies == 0) return PDN_OK;
  PDN_CHECK_ARG(caches && dst && src && len && n_tensors > 0 && n_tensors <= 65535 && n_rows > 0 && n_copies > 0 &&
                    n_copies <= KCP_MAX && max_len > 0 && D > 0 && batch_stride >= (int64_t)max_len * D,
                "pdn_kv_copy_prefix_rows_f32: bad arguments (%d tensors, %d rows of %d, D %d, %d copies)", n_tensors,
                n_rows, max_len, D, n_copies);
  // positions per group: up to 8, so that one long copy still spreads over the device
  const int TP = std::max(1, std::min(8, KCP_MAX / n_copies));
  const int groups = (int)std::min<int64_t>(cdiv64(max_len, TP), 65535);
  const hipStream_t s = (hipStream_t)stream;
  if (D % 4 == 0 && batch_stride % 4 == 0) {
    hipLaunchKernelGGL((kv_copy_prefix_kernel<kcp_f4, 8, 8>), dim3((D / 4 + 7) / 8, groups, n_tensors),
                       dim3(KCP_THREADS), 0, s, caches, batch_stride, n_rows, max_len, D, dst, src, len, n_copies, TP);
  } else {
    hipLaunchKernelGGL((kv_copy_prefix_kernel<float, 16, 16>), dim3((D + 15) / 16, groups, n_tensors),
                       dim3(KCP_THREADS), 0, s, caches, batch_stride, n_rows, max_len, D, dst, src, len, n_copies, TP);
  }
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_PREFIX);
  return PDN_OK;
}
