// Dropout with the mask drawn on the device (nn.Dropout(generator=...), fused.dropout / dropout_add, Llama's embedding and
// residual dropout); the contract is stated in NumPy in core/fused/dropout.py, the ABI in include/pdn_dropout.h.
// Generator: Philox4x32-10.  state = (seed, offset) and slot = the (seed, o) a call claimed, two 64-bit words each, in device
// memory; element i of a call uses word i % 4 of the block for counter o + i / 4 under key seed.
//
//   rng_set_kernel     one thread: the two words of the state.
//   rng_claim_kernel   one thread: slot = state, offset += ceil(n / 4).  The only writer of the state between two sets, and
//                      stream-ordered: no atomics.  A captured step re-runs it at every replay.
//   dropout_kernel<ADD, VEC>
//                      one Philox block feeds one float4: counter index = float4 index, no division anywhere.  A tile is
//                      DR_THREADS * DR_UNROLL float4; a wave owns DR_UNROLL * 64 consecutive ones and a lane carries DR_UNROLL
//                      groups a wave-stride (64 float4 = 1 KiB) apart: every load and store is 16 bytes per lane, coalesced,
//                      all loads of a trip are issued before the first round, and the DR_UNROLL independent ten-round chains
//                      (two 32 x 32 -> 64 products per round: __umulhi and a plain multiply) overlap while they are in
//                      flight.  Grid-stride over tiles, the grid capped at DR_GRID_CAP workgroups.  The last n % 4 elements
//                      take the first words of the block behind the last whole float4, on one thread, as scalars.
//                      VEC = false: x / y not 16-byte aligned (a view that starts inside an array): the same groups as
//                      four scalar accesses each.  ADD: out = residual + dropout(x).
// No LDS, nothing crosses lanes, nothing allocated or read back.  (seed, o) are read from the slot, never passed by value: a
// hipGraph replay sees what its own claim stored.
#include "common.h"

// the statement multiplies and adds in two roundings: no contraction into an fma anywhere in this file
#pragma clang fp contract(off)

#define DR_THREADS 256
#define DR_UNROLL 4
#define DR_GRID_CAP 2048
#define DR_TILE (DR_THREADS * DR_UNROLL)      // float4 groups of one workgroup per trip

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox4x32_10(unsigned long long c, uint32_t k0, uint32_t k1) {
  uint32_t c0 = (uint32_t)c, c1 = (uint32_t)(c >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  return Words{{c0, c1, c2, c3}};
}

template <bool ADD>
__device__ __forceinline__ float drop_one(float x, float r, uint32_t word, uint32_t thr, float s) {
  const float v = word < thr ? 0.0f : __fmul_rn(x, s);
  return ADD ? __fadd_rn(r, v) : v;
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, long long g) {
  if (VEC) return reinterpret_cast<const float4*>(p)[g];
  return make_float4(p[4 * g], p[4 * g + 1], p[4 * g + 2], p[4 * g + 3]);
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, long long g, float4 v) {
  if (VEC) {
    reinterpret_cast<float4*>(p)[g] = v;
  } else {
    p[4 * g] = v.x, p[4 * g + 1] = v.y, p[4 * g + 2] = v.z, p[4 * g + 3] = v.w;
  }
}

__global__ void rng_set_kernel(unsigned long long* __restrict__ state, unsigned long long seed, unsigned long long offset) {
  state[0] = seed;
  state[1] = offset;
}

__global__ void rng_claim_kernel(unsigned long long* __restrict__ state, unsigned long long* __restrict__ slot,
                                 unsigned long long nblocks) {
  const unsigned long long seed = state[0], o = state[1];
  slot[0] = seed;
  slot[1] = o;
  state[1] = o + nblocks;
}

// x, y (and res) hold n floats; nvec = n / 4 whole groups.  x may alias y (each group is read before it is written, by
// the lane that writes it).
template <bool ADD, bool VEC>
__global__ __launch_bounds__(DR_THREADS) void dropout_kernel(const float* x, const float* res, float* y, long long n,
                                                             uint32_t thr, float s,
                                                             const unsigned long long* __restrict__ slot) {
  const unsigned long long seed = slot[0], o = slot[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const long long nvec = n >> 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long in_tile = (long long)wave * (DR_UNROLL * 64) + lane;
  for (long long base = (long long)blockIdx.x * DR_TILE; base < nvec; base += (long long)gridDim.x * DR_TILE) {
    float4 xv[DR_UNROLL], rv[DR_UNROLL];
#pragma unroll
    for (int u = 0; u < DR_UNROLL; ++u) {
      const long long g = base + in_tile + u * 64;
      xv[u] = rv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g < nvec) {
        xv[u] = load4<VEC>(x, g);
        if (ADD) rv[u] = load4<VEC>(res, g);
      }
    }
#pragma unroll
    for (int u = 0; u < DR_UNROLL; ++u) {
      const long long g = base + in_tile + u * 64;
      const Words w = philox4x32_10(o + (unsigned long long)g, k0, k1);
      float4 out;
      out.x = drop_one<ADD>(xv[u].x, rv[u].x, w.w[0], thr, s);
      out.y = drop_one<ADD>(xv[u].y, rv[u].y, w.w[1], thr, s);
      out.z = drop_one<ADD>(xv[u].z, rv[u].z, w.w[2], thr, s);
      out.w = drop_one<ADD>(xv[u].w, rv[u].w, w.w[3], thr, s);
      if (g < nvec) store4<VEC>(y, g, out);
    }
  }
  const int rem = (int)(n & 3);
  if (rem != 0 && blockIdx.x == 0 && threadIdx.x == 0) {          // the ragged tail: the first words of block nvec
    const Words w = philox4x32_10(o + (unsigned long long)nvec, k0, k1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j < rem) {
        const long long i = 4 * nvec + j;
        y[i] = drop_one<ADD>(x[i], ADD ? res[i] : 0.f, w.w[j], thr, s);
      }
    }
  }
}

static int dropout_launch(const char* who, const float* x, const float* res, float* y, int64_t n, double p,
                          const int64_t* slot, bool add, void* stream) {
  if (n == 0) return PDN_OK;
  PDN_CHECK_ARG(x && y && slot && (!add || res) && n > 0, "%s: bad arguments (n %lld)", who, (long long)n);
  PDN_CHECK_ARG(p >= 0.0 && p < 1.0 && (float)p < 1.0f, "%s: p must lie in [0, 1), got %g", who, p);
  PDN_CHECK_ARG(((uintptr_t)x | (uintptr_t)y | (uintptr_t)res | (uintptr_t)slot) % 4 == 0 && (uintptr_t)slot % 8 == 0,
                "%s: misaligned pointer", who);
  const uint32_t thr = (uint32_t)(p * 4294967296.0);               // floor(p * 2^32) < 2^32
  const float s = 1.0f / (1.0f - (float)p);
  const bool vec = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)res) & 15) == 0;
  const int64_t tiles = ((n >> 2) + DR_TILE - 1) / DR_TILE;
  const dim3 grid((unsigned)(tiles < 1 ? 1 : (tiles > DR_GRID_CAP ? DR_GRID_CAP : tiles))), block(DR_THREADS);
  const unsigned long long* sl = (const unsigned long long*)slot;
  hipStream_t st = (hipStream_t)stream;
  if (add) {
    if (vec) hipLaunchKernelGGL((dropout_kernel<true, true>), grid, block, 0, st, x, res, y, (long long)n, thr, s, sl);
    else hipLaunchKernelGGL((dropout_kernel<true, false>), grid, block, 0, st, x, res, y, (long long)n, thr, s, sl);
  } else {
    if (vec) hipLaunchKernelGGL((dropout_kernel<false, true>), grid, block, 0, st, x, res, y, (long long)n, thr, s, sl);
    else hipLaunchKernelGGL((dropout_kernel<false, false>), grid, block, 0, st, x, res, y, (long long)n, thr, s, sl);
  }
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DROPOUT);
  return PDN_OK;
}

extern "C" int pdnd_rng_set(int64_t* state, int64_t seed, int64_t offset, void* stream) {
  PDN_CHECK_ARG(state && (uintptr_t)state % 8 == 0, "pdnd_rng_set: bad state pointer");
  hipLaunchKernelGGL(rng_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long*)state,
                     (unsigned long long)seed, (unsigned long long)offset);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DROPOUT);
  return PDN_OK;
}

extern "C" int pdnd_rng_claim(int64_t* state, int64_t* slot, int64_t n, void* stream) {
  PDN_CHECK_ARG(state && slot && state != slot && (uintptr_t)state % 8 == 0 && (uintptr_t)slot % 8 == 0 && n >= 0,
                "pdnd_rng_claim: bad arguments (n %lld)", (long long)n);
  hipLaunchKernelGGL(rng_claim_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (unsigned long long*)state,
                     (unsigned long long*)slot, ((unsigned long long)n + 3ull) >> 2);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DROPOUT);
  return PDN_OK;
}

extern "C" int pdnd_dropout_fwd_f32(const float* x, float* y, int64_t n, double p, const int64_t* slot, void* stream) {
  return dropout_launch("pdnd_dropout_fwd_f32", x, nullptr, y, n, p, slot, false, stream);
}

extern "C" int pdnd_dropout_bwd_f32(const float* dy, float* dx, int64_t n, double p, const int64_t* slot, void* stream) {
  return dropout_launch("pdnd_dropout_bwd_f32", dy, nullptr, dx, n, p, slot, false, stream);
}

extern "C" int pdnd_dropout_add_fwd_f32(const float* x, const float* residual, float* out, int64_t n, double p,
                                        const int64_t* slot, void* stream) {
  return dropout_launch("pdnd_dropout_add_fwd_f32", x, residual, out, n, p, slot, true, stream);
}
