// Continuous batching (Llama.serve): the prompts admitted into freed decode rows are right-padded to the longest and run
// through one batched causal prompt pass into a staging cache; this copy puts their keys and values into the rows they
// were given.  The decode ticks of a served batch are the SLOTS forms of the ragged ticks (csrc/decode.hip, sample.hip).
#include "common.h"

#define KVS_POS 8      // positions per workgroup

// grid (ceil(Ls / KVS_POS), n_inputs, n_tensors), 256 threads.  Tensor j, input i: positions [0, n_i) of src[j] row i go
// to dst[j] row slots[i], positions [start[i], start[i] + n_i), with n_i = lens[i] clamped to Ls and to the cache
// length.  A position is D contiguous floats on both sides, so a workgroup copies one contiguous run of up to
// KVS_POS * D floats -- as float4s when both ends are 16-byte aligned (uniform per workgroup).  Nothing else is written:
// not the pad positions [n_i, Ls), not any other row, not a row outside [0, n_rows).
__global__ __launch_bounds__(256) void kv_store_slots_kernel(const float* const* __restrict__ src, int64_t src_bs,
                                                             float* const* __restrict__ dst, int64_t dst_bs, int Ls,
                                                             int D, const int* __restrict__ slots,
                                                             const int* __restrict__ lens,
                                                             const int* __restrict__ start, int n_rows, int max_len) {
  const int i = blockIdx.y, j = blockIdx.z;
  const int row = slots[i], s0 = start ? start[i] : 0;
  if (row < 0 || row >= n_rows || s0 < 0) return;
  const int n = min(min(lens[i], Ls), max_len - s0);
  const int t0 = blockIdx.x * KVS_POS, t1 = min(n, t0 + KVS_POS);
  if (t0 >= t1) return;
  const float* s = src[j] + (int64_t)i * src_bs + (int64_t)t0 * D;
  float* d = dst[j] + (int64_t)row * dst_bs + (int64_t)(s0 + t0) * D;
  const int64_t cnt = (int64_t)(t1 - t0) * D;
  if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0 && (cnt & 3) == 0) {
    const float4* s4 = reinterpret_cast<const float4*>(s);
    float4* d4 = reinterpret_cast<float4*>(d);
    for (int64_t e = threadIdx.x; e < cnt / 4; e += 256) d4[e] = s4[e];
  } else {
    for (int64_t e = threadIdx.x; e < cnt; e += 256) d[e] = s[e];
  }
}

extern "C" int pdn_kv_store_slots_f32(const float* const* src, int64_t src_batch_stride, float* const* dst,
                                      int64_t dst_batch_stride, int n_tensors, int n_inputs, int max_src_len, int D,
                                      const int* slots, const int* lens, const int* start, int n_rows, int max_len,
                                      void* stream) {
  if (n_tensors == 0 || n_inputs == 0 || max_src_len == 0) return PDN_OK;
  PDN_CHECK_ARG(src && dst && slots && lens && n_tensors > 0 && n_tensors <= 65535 && n_inputs > 0 &&
                    n_inputs <= 65535 && max_src_len > 0 && D > 0 && n_rows > 0 && max_len > 0 &&
                    src_batch_stride >= 0 && dst_batch_stride >= (int64_t)max_len * D,
                "pdn_kv_store_slots_f32: bad arguments (%d tensors, %d inputs, length %d, D %d, %d rows of %d)",
                n_tensors, n_inputs, max_src_len, D, n_rows, max_len);
  const dim3 grid((max_src_len + KVS_POS - 1) / KVS_POS, n_inputs, n_tensors);
  hipLaunchKernelGGL(kv_store_slots_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, src_batch_stride, dst,
                     dst_batch_stride, max_src_len, D, slots, lens, start, n_rows, max_len);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_SLOTS);
  return PDN_OK;
}
