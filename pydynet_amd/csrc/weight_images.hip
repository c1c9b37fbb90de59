// All weight plane images of a training pass in one launch (include/pdn_wimages.h; gfx950 only).
//
// The split-fp16 products of a layer build the fp16 plane images of their weight per call: rts_w_kernel in front of q | k | v,
// gate | up and dh + SwiGLU backward (csrc/rowtile_split.hip), ors_w_max_kernel + ors_w_img_kernel in front of the
// output-resident products (csrc/outres_split.hip).  In a training step that is 13 launches per layer of 9 .. 48 workgroups
// each, every one directly in front of the product that waits for it.  The weights do not change inside a forward or inside
// a backward pass, so the caller may describe the pass's (weight, form) pairs up front; pdnw_build_kernel then builds every
// image in ONE launch, a workgroup finding its (descriptor, tile or piece chunk, column range) in a job table that travels
// by value (csrc/weight_images_index.h, walked on the host by tests/weight_images_check.cpp).  The device bodies are those
// of the per-call passes (csrc/weight_images.h), so the images are byte-identical; for the output-resident forms a
// workgroup takes its columns' maxima over all pieces itself (a maximum does not depend on the order), which replaces the
// separate maxima launch.
// The products find the images through a thread-local "current set" (pdnw_bind / pdnw_lookup): the key is the W-params
// they would hand their own pass.  Deterministic: fixed order, no atomics.
#include "weight_images.h"
#include "../../include/pdn_wimages.h"
#include <atomic>
#include <vector>

#define PDNW_SM_FLOATS (ORS_W_TILE + 16 * 64)   // >= RTS_W_SM + RTS_W_SMAX
static_assert(PDNW_SM_FLOATS >= RTS_W_SM + RTS_W_SMAX, "the tile body's LDS");
static_assert(sizeof(PdnwDesc) == 64 && sizeof(PdnwTable) <= 3584, "the job table travels by value");

// the images of pieces piece0 .. piece1 - 1, columns 64 y .. of an output-resident form, and (chunk 0) the exponents
template <bool NN>
__device__ __forceinline__ void pdnw_ors(const OrsWParams& p, int y, int chunk, float* sm) {
  const int tid = threadIdx.x, i = pdnw_ors_unit(y, tid);
  const bool on = i < ORS_N * 4;                      // (the last range: 128 threads; the others repeat column 287, unwritten)
  const int d = on ? i >> 2 : ORS_N - 1, q = i & 3;
  float amax = 0.f;
  if (NN) {
    float* cmax = sm + ORS_W_TILE;                    // 16 row groups x 64 columns
    const int c4 = pdnw_nn_max_c4(tid), r0 = pdnw_nn_max_row(tid);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * c4 < pdnw_ors_ncols(y)) {
      for (int k = r0; k < p.np * ORS_KP; k += 16) {
        const float4 a = *reinterpret_cast<const float4*>(p.B + ors_w_src_nn(k / ORS_KP, (k % ORS_KP) * 72 + 16 * y + c4, p.ldb));
        m.x = fmaxf(m.x, ors_finite_or_inf(fabsf(a.x))); m.y = fmaxf(m.y, ors_finite_or_inf(fabsf(a.y)));
        m.z = fmaxf(m.z, ors_finite_or_inf(fabsf(a.z))); m.w = fmaxf(m.w, ors_finite_or_inf(fabsf(a.w)));
      }
    }
    *reinterpret_cast<float4*>(cmax + r0 * 64 + 4 * c4) = m;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) amax = fmaxf(amax, cmax[r * 64 + d - pdnw_ors_col0(y)]);
  } else {
    for (int s = 0; s < p.np; ++s) {
      float v[8];
      ors_w_unit<false>(p, nullptr, s, d, q, v);
      amax = fmaxf(amax, ors_w_max8(v));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));      // the four units of a column lie in four adjacent lanes
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  }
  const int sh = ls_shift(amax);
  if (chunk == 0 && q == 0 && on) p.wsh[d] = sh;
  const int s1 = pdnw_ors_piece1(chunk, p.np);
  for (int s = pdnw_ors_piece0(chunk); s < s1; ++s) {
    if (NN) {
      __syncthreads();                                // the readers of the piece before are through
      ors_w_stage_nn(p, sm, s, 16 * y, pdnw_ors_ncols(y) / 4);
    }
    float v[8];
    ors_w_unit<NN>(p, sm, s, d, q, v);
    if (on) ors_w_put(p.wimg + (int64_t)s * ORS_PIECE, d, q, sh, v);
  }
}

__global__ __launch_bounds__(256) void pdnw_build_kernel(PdnwTable t, char* arena) {
  __shared__ __attribute__((aligned(16))) float sm[PDNW_SM_FLOATS];
  const int j = pdnw_job_of(t, blockIdx.x);
  const PdnwJob& job = t.job[j];
  const int l = blockIdx.x - job.wg0;
  char* img = arena + job.dst;
  if (job.family == PDNW_RTS) {
    RtsWParams p;
    p.B = job.B; p.wimg = img; p.kind = job.kind; p.nper = job.nper; p.ldb = job.ldb; p.bstride = job.bstride;
    p.g_off = job.g_off; p.u_off = job.u_off;
    rts_w_tile(p, l, sm, sm + RTS_W_SM);
    return;
  }
  OrsWParams p;
  p.B = job.B; p.pmax = nullptr; p.wimg = img; p.wsh = reinterpret_cast<int*>(img + (int64_t)job.n * ORS_PIECE);
  p.np = job.n; p.ppb = job.nper; p.ldb = job.ldb; p.bstride = job.bstride;
  if (job.family == PDNW_ORS_NN) pdnw_ors<true>(p, pdnw_ors_colrange(l), pdnw_ors_chunk(l), sm);
  else pdnw_ors<false>(p, pdnw_ors_colrange(l), pdnw_ors_chunk(l), sm);
}

// ---- host side ----------------------------------------------------------------------------------------------------
namespace {
struct PdnwBound {
  std::vector<PdnwDesc> descs;
  std::vector<int64_t> off;
  char* arena = nullptr;
  void* stream = nullptr;
  bool on = false;
};
thread_local PdnwBound t_bound;
std::atomic<int64_t> g_builds{0}, g_hits{0}, g_passes{0};

bool pdnw_set_ok(const PdnwDesc* d, int n) {
  if (!d || n < 1) return false;
  for (int i = 0; i < n; ++i)
    if (!pdnw_desc_ok(d[i])) return false;
  return true;
}
bool al16p(const void* p) { return ((uintptr_t)p & 15) == 0; }
}

bool pdnw_lookup(const PdnwDesc& key, void* stream, char** img, int** wsh) {
  const PdnwBound& b = t_bound;
  if (b.on && b.stream == stream) {
    for (size_t i = 0; i < b.descs.size(); ++i) {
      if (!pdnw_same(b.descs[i], key)) continue;
      *img = b.arena + b.off[i];
      if (wsh) *wsh = reinterpret_cast<int*>(*img + pdnw_exp_offset(key));
      g_hits.fetch_add(1, std::memory_order_relaxed);
      return true;
    }
  }
  g_passes.fetch_add(1, std::memory_order_relaxed);
  return false;
}

extern "C" int64_t pdnw_desc_bytes(void) { return (int64_t)sizeof(PdnwDesc); }

extern "C" int pdnw_desc_qkv(void* desc, const float* wq, int64_t w_stride, int D, int K) {
  PDN_CHECK_ARG(desc && wq && K == RTS_K && D >= 32 && D % 32 == 0 && w_stride % 4 == 0 && al16p(wq),
                "pdnw_desc_qkv: K 288, D a multiple of 32, w_stride a multiple of 4, 16-byte aligned weights");
  *static_cast<PdnwDesc*>(desc) = pdnw_desc_of_qkv(wq, w_stride, D);
  return PDN_OK;
}
extern "C" int pdnw_desc_gateup(void* desc, const float* w_gate, int64_t w_stride, int F, int K) {
  const int64_t ws = w_stride < 0 ? -w_stride : w_stride;
  PDN_CHECK_ARG(desc && w_gate && K == RTS_K && F >= 16 && F % 16 == 0 && ws % 4 == 0 && ws >= (int64_t)K * F &&
                    ws + (int64_t)K * F < (1ll << 30) && al16p(w_gate),
                "pdnw_desc_gateup: K 288, F a multiple of 16, the matrices apart and within 2^30 floats");
  *static_cast<PdnwDesc*>(desc) = pdnw_desc_of_gateup(w_gate, w_stride, F);
  return PDN_OK;
}
extern "C" int pdnw_desc_down_t(void* desc, const float* w_down, int F, int K) {
  PDN_CHECK_ARG(desc && w_down && K == RTS_K && F >= 32 && F % 32 == 0 && al16p(w_down), "pdnw_desc_down_t: K 288, F a multiple of 32");
  *static_cast<PdnwDesc*>(desc) = pdnw_desc_of_down_t(w_down, F, K);
  return PDN_OK;
}
extern "C" int pdnw_desc_outres(void* desc, const float* B, int K, int64_t ldb, int b_trans, int kb, int64_t b_bstride) {
  PDN_CHECK_ARG(desc && B && K >= ORS_MIN_K && K <= ORS_MAX_K && K % ORS_KP == 0 && (ldb & 3) == 0 && (b_bstride & 3) == 0 && al16p(B) &&
                    (kb > 0 ? (b_trans && kb % ORS_KP == 0 && K % kb == 0 && ldb >= kb) : ldb >= (b_trans ? K : ORS_N)),
                "pdnw_desc_outres: K a multiple of 32 in 256 .. 4096, strides multiples of 4, blocks only transposed");
  *static_cast<PdnwDesc*>(desc) = pdnw_key_ors(B, K, ldb, b_trans, kb, b_bstride);
  return PDN_OK;
}

extern "C" int64_t pdnw_set_bytes(const void* descs, int n) {
  const PdnwDesc* d = static_cast<const PdnwDesc*>(descs);
  return pdnw_set_ok(d, n) ? pdnw_offset(d, n) : 0;
}

extern "C" int pdnw_set_build(const void* descs, int n, void* arena, void* stream) {
  const PdnwDesc* d = static_cast<const PdnwDesc*>(descs);
  PDN_CHECK_ARG(pdnw_set_ok(d, n) && arena && ((uintptr_t)arena % PDNW_ALIGN) == 0, "pdnw_set_build: bad descriptors or arena");
  for (int first = 0; first < n; first += PDNW_MAX_DESCS) {
    PdnwTable t;
    memset(&t, 0, sizeof(t));
    pdnw_table(d, first, n - first < PDNW_MAX_DESCS ? n - first : PDNW_MAX_DESCS, &t);
    hipLaunchKernelGGL(pdnw_build_kernel, dim3((unsigned)t.nwgs), dim3(256), 0, (hipStream_t)stream, t, static_cast<char*>(arena));
    g_builds.fetch_add(1, std::memory_order_relaxed);
  }
  PDN_LAUNCH_CHECK();
  return PDN_OK;
}

// PDN_WIMAGES=0: read on EVERY call (a test switches it in process), announced the first time it is seen at 0
extern "C" int pdnw_bind(const void* descs, int n, void* arena, void* stream) {
  const PdnwDesc* d = static_cast<const PdnwDesc*>(descs);
  PDN_CHECK_ARG(pdnw_set_ok(d, n) && arena && ((uintptr_t)arena % PDNW_ALIGN) == 0, "pdnw_bind: bad descriptors or arena");
  PdnwBound& b = t_bound;
  b.on = false;
  const char* e = getenv("PDN_WIMAGES");
  if (e && atoi(e) == 0) {
    static bool s_told = false;
    if (!s_told) {
      s_told = true;
      fprintf(stderr, "[pdnhip] WARNING: PDN_WIMAGES=0 -- every split-fp16 product builds its weight images per call\n");
    }
    return PDN_OK;
  }
  b.descs.assign(d, d + n);
  b.off.resize(n);
  int64_t o = 0;
  for (int i = 0; i < n; ++i) { b.off[i] = o; o += pdnw_round_up(pdnw_image_bytes(d[i])); }
  b.arena = static_cast<char*>(arena); b.stream = stream; b.on = true;
  return PDN_OK;
}
extern "C" int pdnw_unbind(void) {
  t_bound.on = false;
  t_bound.arena = nullptr;
  return PDN_OK;
}
extern "C" int pdnw_stats(int64_t* builds, int64_t* hits, int64_t* passes, int reset) {
  if (builds) *builds = g_builds.load();
  if (hits) *hits = g_hits.load();
  if (passes) *passes = g_passes.load();
  if (reset) { g_builds = 0; g_hits = 0; g_passes = 0; }
  return PDN_OK;
}
