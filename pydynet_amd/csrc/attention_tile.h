// Device helpers shared by the streaming attention kernels (attention_stream.hip) and the grouped-query kernels
// (attention_gqa.hip): the argument block, the register-staged 32-row tile loader of the LDS ring, the additive terms of a
// score and the transposed accumulator store.  The scheme they serve is described at the top of attention_stream.hip.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define AS_LD(hd) ((hd) + 4)

struct AttnArgs {
  int H, Lq, Lk, causal, start_pos;
  int64_t q_rs, q_bs, kv_rs, kv_bs;            // row / batch strides (floats) of q,o,dq and of k,v,dk,dv
  float inv_sqrt;
  const float* mask;                            // additive, element (b, h, q, k) at b*m_b + h*m_h + q*m_q + k*m_k
  int64_t m_b, m_h, m_q, m_k;
  const float* rc;                              // RoPE tables (positions x hd/2), rotate q and k rows on load
  const float* rs;
};

__device__ __forceinline__ int as_krow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

__device__ __forceinline__ float4 as_rot(float4 v, const float* __restrict__ cs, const float* __restrict__ sn,
                                         int pos, int pair0, int half, float sign) {
  const float2 c = *reinterpret_cast<const float2*>(cs + (int64_t)pos * half + pair0);
  float2 s = *reinterpret_cast<const float2*>(sn + (int64_t)pos * half + pair0);
  s.x *= sign; s.y *= sign;
  float4 o;
  o.x = v.x * c.x - v.y * s.x; o.y = v.x * s.x + v.y * c.x;
  o.z = v.z * c.y - v.w * s.y; o.w = v.z * s.y + v.w * c.y;
  return o;
}

// Register-staged loader of one 32-row tile of TWO [rows][HD] matrices (row stride rs floats) into two
// padded LDS images [32][HD+4].  Rows >= n_rows read as zero.  rot0: rotate matrix 0 rows (RoPE).
template <int HD>
struct TileLoader {
  static constexpr int F4 = HD / 4, PIECES = 32 * F4, NP = (PIECES + 255) / 256;
  float4 r0[NP], r1[NP];
  __device__ __forceinline__ void issue(const float* __restrict__ g0, const float* __restrict__ g1, int64_t rs,
                                        int row0, int n_rows, const float* __restrict__ rc,
                                        const float* __restrict__ rsn, bool rot0) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int u = threadIdx.x + 256 * j;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
      if (u < PIECES) {
        const int row = u / F4, c4 = u - row * F4;
        if (row0 + row < n_rows) {
          a = *reinterpret_cast<const float4*>(g0 + (int64_t)(row0 + row) * rs + 4 * c4);
          c = *reinterpret_cast<const float4*>(g1 + (int64_t)(row0 + row) * rs + 4 * c4);
          if (rc && rot0) a = as_rot(a, rc, rsn, row0 + row, 2 * c4, HD / 2, 1.f);
        }
      }
      r0[j].x = a.x; r0[j].y = a.y; r0[j].z = a.z; r0[j].w = a.w;
      r1[j].x = c.x; r1[j].y = c.y; r1[j].z = c.z; r1[j].w = c.w;
    }
  }
  __device__ __forceinline__ void commit(float* __restrict__ s0, float* __restrict__ s1) {
    constexpr int LD = AS_LD(HD);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int u = threadIdx.x + 256 * j;
      if (u < PIECES) {
        const int row = u / F4, c4 = u - row * F4;
        *reinterpret_cast<float4*>(s0 + row * LD + 4 * c4) = r0[j];
        *reinterpret_cast<float4*>(s1 + row * LD + 4 * c4) = r1[j];
      }
    }
  }
};

// additive terms of one score register: -inf for keys past the end / after the query (causal), plus the mask
__device__ __forceinline__ float as_bias(const AttnArgs& a, const float* __restrict__ mrow, int q, int key) {
  if (key >= a.Lk || (a.causal && key > q + a.start_pos)) return -INFINITY;
  return mrow ? mrow[(int64_t)key * a.m_k] : 0.f;
}

// number of 32-key tiles a block of queries [q0, q1) can see
__device__ __forceinline__ int as_key_tiles(const AttnArgs& a, int q1) {
  int last = a.Lk - 1;
  if (a.causal) last = min(last, q1 - 1 + a.start_pos);
  return last < 0 ? 0 : last / 32 + 1;
}

// X^T[d][row] accumulators (lane = row, registers = d) -> [row][d] through LDS -> coalesced row stores
template <int HD, int DT>
__device__ __forceinline__ void as_store_T(float* __restrict__ slot, const f32x16 (&t)[DT], float* __restrict__ dst,
                                           int64_t rs, int row0, int n_rows, int li, int lh, int lane,
                                           const float* __restrict__ rc, const float* __restrict__ rsn, int pos0) {
  constexpr int LD = AS_LD(HD), F4 = HD / 4;
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int dd = d * 32 + as_krow(r, lh);
      if (dd < HD) slot[li * LD + dd] = t[d][r];
    }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  for (int u = lane; u < 32 * F4; u += 64) {
    const int row = u / F4, c4 = u - row * F4;
    if (row0 + row < n_rows) {
      float4 v = *reinterpret_cast<const float4*>(slot + row * LD + 4 * c4);
      if (rc) v = as_rot(v, rc, rsn, pos0 + row0 + row, 2 * c4, HD / 2, -1.f);     // gradient of RoPE
      *reinterpret_cast<float4*>(dst + (int64_t)(row0 + row) * rs + 4 * c4) = v;
    }
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
}
