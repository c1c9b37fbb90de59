// The per-row sampler of sample.hip as device code (the contract is stated at the top of sample.hip): shared by
// the single-workgroup ticks there and the workgroup-per-row ticks of decode_wide.hip, so that both draw the same
// token from the same logits and counter.
#pragma once
#include <stddef.h>

#include "common.h"

// include/pdn_hip.h: pdn_sample_params (the header is C and is not included by the kernels)
struct SampleParams {
  float temperature;
  int top_k;
  float top_p;
  float min_p;                                       // (the former padding: 0 = off; read by the per-row launches only)
  uint64_t seed;
};
static_assert(sizeof(SampleParams) == 24 && offsetof(SampleParams, min_p) == 12 && offsetof(SampleParams, seed) == 16,
              "pdn_sample_params layout");

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)
#define SMP_BINS 4096

struct SmpShared {
  unsigned long long hist[SMP_BINS];
  unsigned long long wtot[SMP_WAVES];
  float fmax[SMP_WAVES];
  int farg[SMP_WAVES];
  unsigned sel;
  unsigned long long sel_above;
  int tok;
};

// order-preserving: a < b (as floats, no NaN) <=> key(a) < key(b)
__device__ __forceinline__ unsigned smp_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Philox4x64-10 (Salmon et al., SC'11), first word of the block for counter (c0, c1, 0, 0) and key (k0, 0)
__device__ __forceinline__ uint64_t smp_philox_w0(uint64_t c0, uint64_t c1, uint64_t k0) {
  uint64_t c2 = 0, c3 = 0, k1 = 0;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
    const uint64_t hi0 = __umul64hi(0xD2E7470EE14C6C93ull, c0), lo0 = 0xD2E7470EE14C6C93ull * c0;
    const uint64_t hi1 = __umul64hi(0xCA5A826395121157ull, c2), lo1 = 0xCA5A826395121157ull * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
  }
  return c0;
}

// integer weight of a logit: exp((z - m) / T) in [0, 1] scaled by 2^40 (NaN -> 0)
__device__ __forceinline__ unsigned long long smp_weight(float z, float m, float T) {
  const float e = expf((z - m) / T);
  return e >= 0.f ? (unsigned long long)(e * 1099511627776.f) : 0ull;
}

// inclusive scan of one value per thread over the workgroup (in thread order); *total = the sum of all
__device__ __forceinline__ unsigned long long smp_scan(unsigned long long v, SmpShared& s, unsigned long long* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  if (lane == 63) s.wtot[wave] = v;
  __syncthreads();
  unsigned long long off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < SMP_WAVES; ++w) {
    const unsigned long long x = s.wtot[w];
    off += w < wave ? x : 0ull;
    tot += x;
  }
  __syncthreads();                                   // (wtot is rewritten by the next scan)
  *total = tot;
  return v + off;
}

// The largest key K such that the weight of {i : key_i >= K, key_i >= floor} is at least `need` (MASS: weights w_i and
// need = ceil(p * total weight above floor); else counts and need = k).  Levels of 12, 12 and 8 key bits.
template <bool MASS>
__device__ __forceinline__ unsigned smp_select(const float* __restrict__ row, int V, unsigned floor, float m, float T,
                                               float p, unsigned long long need, SmpShared& s) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, pmask = 0;
  unsigned long long above = 0;                      // weight of the keys above the current prefix's range
#pragma unroll 1
  for (int lv = 0; lv < 3; ++lv) {
    const int sh = lv == 0 ? 20 : lv == 1 ? 8 : 0;
    const unsigned nb = lv == 2 ? 256u : 4096u;
    for (int i = tid; i < SMP_BINS; i += SMP_THREADS) s.hist[i] = 0;
    if (tid == 0) { s.sel = 0; s.sel_above = above; }     // (only a row with NaNs can leave these in place)
    __syncthreads();
    for (int i = tid; i < V; i += SMP_THREADS) {
      const float z = row[i];
      const unsigned k = smp_key(z);
      if (k >= floor && (k & pmask) == prefix) {
        const unsigned long long w = MASS ? smp_weight(z, m, T) : 1ull;
        if (w) atomicAdd(&s.hist[(k >> sh) & (nb - 1)], w);      // integer: the sum does not depend on the order
      }
    }
    __syncthreads();
    // thread t owns bins nb-1-4t .. nb-4-4t: a scan in thread order is a suffix sum over the bins
    unsigned long long h[4], part = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int bin = (int)nb - 1 - 4 * tid - q;
      h[q] = bin >= 0 ? s.hist[bin] : 0ull;
      part += h[q];
    }
    unsigned long long tot;
    const unsigned long long incl = smp_scan(part, s, &tot);
    if (MASS && lv == 0) {
      // tot = the mass of every token above the floor (the kept set of step 1)
      const double want = ceil((double)p * (double)tot);
      need = want < 1.0 ? 1ull : want >= (double)tot ? tot : (unsigned long long)want;
    }
    unsigned long long run = above + incl - part;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int bin = (int)nb - 1 - 4 * tid - q;
      if (bin >= 0 && run < need && run + h[q] >= need) { s.sel = (unsigned)bin; s.sel_above = run; }
      run += h[q];
    }
    __syncthreads();
    prefix |= s.sel << sh;
    pmask |= (nb - 1) << sh;
    above = s.sel_above;
    __syncthreads();                                 // (sel is rewritten by the next level)
  }
  return prefix;
}

// The draw of smp_row: chunk sums, block scan, the chunk holding the target is walked by its thread.  MINP: both the chunk
// sums and the walk skip a token whose integer weight is below `wmin` (MINP = false is the draw of before min_p, instruction
// for instruction).  `arg`: the row's first maximum, the token of a row whose kept mass is 0 (only with NaNs).
template <bool MINP>
__device__ __forceinline__ int smp_draw(const float* __restrict__ row, int V, unsigned floor, float mx, float T,
                                        unsigned long long wmin, uint64_t t, uint64_t b, uint64_t seed, int arg,
                                        SmpShared& s) {
  const int tid = threadIdx.x;
  const int C = (V + SMP_THREADS - 1) / SMP_THREADS;
  const int lo = min(tid * C, V), hi = min(lo + C, V);
  unsigned long long part = 0;
  for (int i = lo; i < hi; ++i) {
    const float z = row[i];
    if (smp_key(z) >= floor) {
      const unsigned long long w = smp_weight(z, mx, T);
      if (!MINP || w >= wmin) part += w;
    }
  }
  if (tid == 0) s.tok = arg;
  unsigned long long W;
  const unsigned long long incl = smp_scan(part, s, &W);
  // u * W with u = r * 2^-24: the token is the first whose inclusive prefix exceeds floor(r * W / 2^24)
  const unsigned long long r = smp_philox_w0(t, b, seed) >> 40;
  const unsigned long long target = r * (W >> 24) + ((r * (W & 0xFFFFFFull)) >> 24);
  const unsigned long long excl = incl - part;
  if (W > 0 && excl <= target && target < incl) {
    unsigned long long run = excl;
    for (int i = lo; i < hi; ++i) {
      const float z = row[i];
      if (smp_key(z) >= floor) {
        const unsigned long long w = smp_weight(z, mx, T);
        if (!MINP || w >= wmin) {
          run += w;
          if (run > target) { s.tok = i; break; }
        }
      }
    }
  }
  __syncthreads();
  return s.tok;
}

// the sampled token of one row (every thread of the workgroup calls it and gets the token).  MINP: the block's min_p is
// honoured (the per-row launches of include/pdn_persample.h); MINP = false is the sampler of before, which never reads it
// (the shared-parameter launches, whose callers write 0 there).
template <bool MINP = false>
__device__ __forceinline__ int smp_row(const float* __restrict__ row, int V, const SampleParams prm, uint64_t t,
                                       uint64_t b, SmpShared& s) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // max and its first index
  float mx = -INFINITY;
  int arg = 0x7fffffff;
  for (int i = tid; i < V; i += SMP_THREADS) {
    const float z = row[i];
    if (z > mx) { mx = z; arg = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(mx, o, 64);
    const int oi = __shfl_xor(arg, o, 64);
    if (ov > mx || (ov == mx && oi < arg)) { mx = ov; arg = oi; }
  }
  if (lane == 0) { s.fmax[wave] = mx; s.farg[wave] = arg; }
  __syncthreads();
  mx = s.fmax[0]; arg = s.farg[0];
#pragma unroll
  for (int w = 1; w < SMP_WAVES; ++w)
    if (s.fmax[w] > mx || (s.fmax[w] == mx && s.farg[w] < arg)) { mx = s.fmax[w]; arg = s.farg[w]; }
  if (arg == 0x7fffffff) arg = 0;                    // (a row of NaNs: token 0, as numpy.argmax)
  const float T = prm.temperature;
  if (!(T > 0.f)) {                                   // (uniform) a greedy request among sampled ones: its first maximum
    __syncthreads();                                  // (fmax / farg are rewritten by the next row of a one-workgroup tick)
    return arg;
  }

  unsigned floor = 0;
  if (prm.top_k > 0 && prm.top_k < V) floor = smp_select<false>(row, V, 0u, mx, T, 1.f, (unsigned long long)prm.top_k, s);
  if (prm.top_p < 1.f) floor = smp_select<true>(row, V, floor, mx, T, prm.top_p, 0ull, s);

  // min_p (include/pdn_persample.h): of the tokens kept so far, those whose weight is below min_p times the largest (the
  // maximum's, 2^40) leave the draw.  The threshold in the weights' integer units, once per row; min_p = 0 (off) takes the
  // draw of before (uniform over the workgroup: every thread holds the same block).
  if (MINP && prm.min_p > 0.f)
    return smp_draw<true>(row, V, floor, mx, T, (unsigned long long)(prm.min_p * 1099511627776.f), t, b, prm.seed, arg, s);
  return smp_draw<false>(row, V, floor, mx, T, 0ull, t, b, prm.seed, arg, s);
}
