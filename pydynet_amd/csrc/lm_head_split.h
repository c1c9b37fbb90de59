// What the split-fp16 lm_head kernels share (csrc/lm_head_split.hip: forward, csrc/lm_head_dx_split.hip: input gradient):
// the library switches, the power-of-two scale of a row / column and the split of a scaled fp32 value into two fp16 planes,
//   a * 2^s = h + l / 2048,   h = fp16(a * 2^s),  l = fp16((a * 2^s - h) * 2048)        (22 significant bits).
#pragma once
#include "common.h"
#include <stdlib.h>

// A/B and timing-ablation switches, read ONCE per process and announced when they differ from the default.
static int ls_env_switch(const char* name, int dflt, const char* what) {
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  if (v != dflt) fprintf(stderr, "[pdnhip] WARNING: %s=%d -- %s\n", name, v, what);
  return v;
}

// the exponent that puts `amax` into [2^8, 2^9); 0 for an all-zero and for a non-finite row / column (whose Inf / NaN
// then reach the product as they are: its results come out non-finite like those of the fp32 kernel).
// frexp: amax = f 2^E, f in [0.5, 1), subnormals included, so the result lies in [-119, 157]: clamped by construction,
// and applied by ldexp -- 2^157 is never formed as a float.
__device__ __forceinline__ int ls_shift(float amax) {
  if (!(amax < INFINITY) || amax == 0.f) return 0;
  int E;
  (void)frexpf(amax, &E);
  return 9 - E;
}
// the two planes of a value that is scaled already
__device__ __forceinline__ void ls_split_scaled(float t, _Float16& h, _Float16& l) {
  h = (_Float16)t;
  l = (_Float16)((t - (float)h) * 2048.f);
}
__device__ __forceinline__ void ls_split(float a, int sh, _Float16& h, _Float16& l) { ls_split_scaled(ldexpf(a, sh), h, l); }
