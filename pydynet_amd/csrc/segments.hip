// Document bounds of packed rows (include/pdn_segattn.h: pdns_segment_bounds_i32; statement:
// pydynet_amd/core/fused/segments.py).  seg: (B, L) int32, non-decreasing along a row, equal ids = one document.
//   start[b][i] = smallest j with seg[b][j] == seg[b][i]        end[b][i] = one past the largest such j
// One workgroup per row.  A position that opens a run contributes its index to a running MAXIMUM (start), a position
// that closes one contributes index + 1 to a running MINIMUM taken from the right (end); both scans run over the row in
// LDS, log2(L) doubling steps.  A row that decreases somewhere raises *err_flag and gets the bounds of plain causal
// attention (start 0, end L): the step goes on with defined values and the host finds the flag at its next check.
// The bounds are made on the device so that a captured step follows an id buffer whose contents change between replays.
#include "common.h"

#define SEGB_THREADS 256
#define SEGB_MAX_L 4096
#define SEGB_PER (SEGB_MAX_L / SEGB_THREADS)

__global__ __launch_bounds__(SEGB_THREADS) void segment_bounds_kernel(const int* __restrict__ seg, int L, int* __restrict__ start,
                                                                      int* __restrict__ end, int* __restrict__ err) {
  __shared__ int s_lo[SEGB_MAX_L], s_hi[SEGB_MAX_L];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int* row = seg + (int64_t)blockIdx.x * L;
  if (tid == 0) bad = 0;
  __syncthreads();
  bool mine = false;
  for (int i = tid; i < L; i += SEGB_THREADS) {
    const int v = row[i];
    const int prev = i > 0 ? row[i - 1] : v, next = i + 1 < L ? row[i + 1] : v;
    if (v < prev) mine = true;
    s_lo[i] = (i == 0 || v != prev) ? i : 0;
    s_hi[i] = (i + 1 == L || v != next) ? i + 1 : L;
  }
  if (mine) bad = 1;
  __syncthreads();
  for (int d = 1; d < L; d <<= 1) {
    int a[SEGB_PER], c[SEGB_PER];
#pragma unroll
    for (int j = 0; j < SEGB_PER; ++j) {
      const int i = tid + SEGB_THREADS * j;
      if (i < L) {
        a[j] = max(s_lo[i], i >= d ? s_lo[i - d] : 0);
        c[j] = min(s_hi[i], i + d < L ? s_hi[i + d] : L);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SEGB_PER; ++j) {
      const int i = tid + SEGB_THREADS * j;
      if (i < L) { s_lo[i] = a[j]; s_hi[i] = c[j]; }
    }
    __syncthreads();
  }
  const bool b = bad != 0;
  for (int i = tid; i < L; i += SEGB_THREADS) {
    start[(int64_t)blockIdx.x * L + i] = b ? 0 : s_lo[i];
    end[(int64_t)blockIdx.x * L + i] = b ? L : s_hi[i];
  }
  if (b && tid == 0) *err = 1;
}

extern "C" int pdns_segment_bounds_i32(const int* seg_ids, int B, int L, int* seg_start, int* seg_end, int* err_flag,
                                       void* stream) {
  if (B == 0 || L == 0) return PDN_OK;
  PDN_CHECK_ARG(seg_ids && seg_start && seg_end && err_flag && B > 0 && L > 0, "pdns_segment_bounds_i32: bad arguments");
  if (L > SEGB_MAX_L) {
    pdn_set_error("pdns_segment_bounds_i32: rows of up to %d positions", SEGB_MAX_L);
    return PDN_EUNSUPPORTED;
  }
  hipLaunchKernelGGL(segment_bounds_kernel, dim3((unsigned)B), dim3(SEGB_THREADS), 0, (hipStream_t)stream, seg_ids, L, seg_start,
                     seg_end, err_flag);
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}
