// Wide decode step: the graph-replayed decode of csrc/decode.hip for 9 <= B <= 256 rows (Llama.generate,
// generate_ragged and serve past the B <= 8 plan).  Per layer 5 launches: q | k | v (RMSNorm in the load), the per-row
// attention of decode.hip (pdn_decode_attention_rows_f32), the output projection (merge of the key-range partials in
// the load, x += in the epilogue), gate | up (RMSNorm in the load) and down (SwiGLU in the load, x += in the epilogue);
// then the vocabulary projection and one tick.
//
// The product y (B x N) = A(x) (B x K) @ W (K x N) runs on fp32 MFMA (v_mfma_f32_32x32x2_f32, f32 products accumulated
// in f32; the tests bound its error against float64, they do not compare it bit for bit with a VALU fmaf chain).  A workgroup owns a 32-column tile of W and EVERY row, so each
// weight is read once per launch; the rows of a 32-wide contraction chunk are staged in LDS ([k][row]: a lane's A
// operand A[row = lane & 31][k = lane >> 5] is a conflict-free read), transformed on the way (RMSNorm weight / SwiGLU /
// attention-partial merge).  The four waves take interleaved k-steps of the chunk and are summed in a fixed order.
// Narrow outputs (N = D: 9 column tiles) cannot fill the chip, so the contraction is split over a second grid
// dimension: every split stores its partial tile, and the workgroup that arrives last at the tile's counter (agent-scope
// release / acquire) sums the partials in split order 0, 1, ... -- the result does not depend on which one that is, and
// there are no float atomics, so two launches give the same bits.  The counters sit in a region of fixed size at the
// start of the workspace, the same for every shape, so that the launches of a step can share one workspace: each
// counter is put back to zero by its last arriver, and no launch writes partial tiles over another shape's counters.
#include "common.h"
#include "sample_row.h"

#define WD_MAX_B 256
#define WD_TN 32                 // output columns per workgroup
#define WD_KC 32                 // contraction chunk staged per pass (16 MFMA k-steps, 4 per wave)
#define WD_MAX_NS 8              // key-range partials merged in the load (mode 3)
#define WD_COUNTERS 192          // arrival counters at the start of the workspace: a split is only taken below 192 tiles

typedef float wd_f32x16 __attribute__((ext_vector_type(16)));

// contraction splits for a (K, N) product: one split when the column tiles alone cover the chip, else enough splits of
// whole chunks to give ~256 workgroups.  Chunks per split: wd_per.
static int wd_per(int K, int N) {
  const int T = (N + WD_TN - 1) / WD_TN, nch = (K + WD_KC - 1) / WD_KC;
  if (T >= WD_COUNTERS) return nch;
  int ks = (256 + T - 1) / T;
  if (ks > nch) ks = nch;
  return (nch + ks - 1) / ks;
}
static int wd_splits(int K, int N) {
  const int nch = (K + WD_KC - 1) / WD_KC, per = wd_per(K, N);
  return (nch + per - 1) / per;
}

// MODE 0: A = x; 1: A = RMSNorm(x) (the weight in the load, the row's 1 / rms in the epilogue); 2: A = silu(gate) * up
// of [gate | up] rows of width 2 K; 3: A = the merge of `ns` key-range partials of pdn_decode_attention_rows_f32 per row.
// EPI 0: y = acc (+ bias); 1: y += acc (+ bias); 2: as 0, plus the first maximum of the tile's columns per row.
template <int MT, int MODE>
__global__ __launch_bounds__(256) void wide_gemm_kernel(const float* __restrict__ x, int64_t x_rs,
                                                        const float* __restrict__ norm_w, float eps, int ns, int hd,
                                                        const float* __restrict__ W, int64_t w_rs, int blk_cols,
                                                        int64_t w_bs, const float* __restrict__ bias, float* y,
                                                        int64_t y_rs, int epi, float* __restrict__ cand_v,
                                                        int* __restrict__ cand_i, const int* __restrict__ pos, int B,
                                                        int K, int N, int per, float* work) {
  constexpr int R = 32 * MT;                                      // rows, padded to the MFMA tile
  __shared__ __attribute__((aligned(16))) float as[WD_KC * R];    // A chunk [k][row]; after the loop [row][col] results
  __shared__ float ssq[R];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile = blockIdx.x, split = blockIdx.y, KS = gridDim.y, T = gridDim.x;
  const int n0 = tile * WD_TN;
  const int nch = (K + WD_KC - 1) / WD_KC, c0 = split * per, c1 = min(c0 + per, nch);

  // the weight column of this lane (columns past N read the last column, zeroed)
  const int n = n0 + (lane & 31);
  const bool ncol = n < N;
  const int nc = ncol ? n : N - 1, blk = nc / blk_cols;
  const float* wcol = W + blk * w_bs + (nc - blk * blk_cols);
  // the row this thread stages (rows past B and stopped rows: zeros, no loads)
  const int r = tid;
  const bool live = r < B && (pos == nullptr || pos[r] >= 0);
  const float* xr = x + (int64_t)(live ? r : 0) * x_rs;
  float ss = 0.f;

  wd_f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;

  for (int c = c0; c < c1; ++c) {
    const int kb = c * WD_KC;
    // the weights of this wave's k-steps first: they travel while the rows are staged
    float wv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = kb + 2 * (wave + 4 * i) + (lane >> 5);
      wv[i] = wcol[(int64_t)(k < K ? k : K - 1) * w_rs];
      if (!ncol || k >= K) wv[i] = 0.f;
    }
    __syncthreads();                                              // (the previous chunk's MFMAs are done with `as`)
    if (r < R) {
      float* dst = as + r;
#pragma unroll 2
      for (int q = 0; q < WD_KC / 4; ++q) {
        const int k = kb + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live && k < K) {
          if (MODE == 0 || MODE == 1) {
            v = *reinterpret_cast<const float4*>(xr + k);
            if (MODE == 1) {
              ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
              const float4 g = *reinterpret_cast<const float4*>(norm_w + k);
              v.x *= g.x; v.y *= g.y; v.z *= g.z; v.w *= g.w;
            }
          } else if (MODE == 2) {
            const float4 g = *reinterpret_cast<const float4*>(xr + k);
            const float4 u = *reinterpret_cast<const float4*>(xr + K + k);
            v.x = g.x / (1.f + expf(-g.x)) * u.x; v.y = g.y / (1.f + expf(-g.y)) * u.y;
            v.z = g.z / (1.f + expf(-g.z)) * u.z; v.w = g.w / (1.f + expf(-g.w)) * u.w;
          } else {
            // record (split s, head h) at ((s * H + h) * (4 + hd)): [m, l, -, - | o[hd]] (unnormalised o);
            // att = sum_s exp(m_s - M) o_s / sum_s exp(m_s - M) l_s over the splits with keys (l > 0)
            const int H = K / hd, rec = 4 + hd, h = k / hd, d = k - h * hd;
            float M = -INFINITY;
#pragma unroll
            for (int s = 0; s < WD_MAX_NS; ++s)
              if (s < ns) {
                const float* rr = xr + (int64_t)(s * H + h) * rec;
                if (rr[1] > 0.f) M = fmaxf(M, rr[0]);
              }
            float wsp[WD_MAX_NS], den = 0.f;
#pragma unroll
            for (int s = 0; s < WD_MAX_NS; ++s) {
              wsp[s] = 0.f;
              if (s < ns) {
                const float* rr = xr + (int64_t)(s * H + h) * rec;
                wsp[s] = rr[1] > 0.f ? expf(rr[0] - M) : 0.f;
                den += wsp[s] * rr[1];
              }
            }
            const float inv = 1.f / den;
#pragma unroll
            for (int s = 0; s < WD_MAX_NS; ++s)
              if (s < ns) {
                const float w = wsp[s] * inv;
                const float4 o = *reinterpret_cast<const float4*>(xr + (int64_t)(s * H + h) * rec + 4 + d);
                v.x = fmaf(w, o.x, v.x); v.y = fmaf(w, o.y, v.y); v.z = fmaf(w, o.z, v.z); v.w = fmaf(w, o.w, v.w);
              }
          }
        }
        dst[(4 * q + 0) * R] = v.x; dst[(4 * q + 1) * R] = v.y; dst[(4 * q + 2) * R] = v.z; dst[(4 * q + 3) * R] = v.w;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int kk = 2 * (wave + 4 * i) + (lane >> 5);
#pragma unroll
      for (int m = 0; m < MT; ++m)
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kk * R + m * 32 + (lane & 31)], wv[i], acc[m], 0, 0, 0);
    }
  }

  // ---- the four waves' k-steps, summed in wave order into red [row][col] (D layout of 32x32x2: column lane & 31,
  //      row (e & 3) + 8 (e >> 2) + 4 (lane >> 5)) ----
  float* red = as;
  if (MODE == 1 && r < R) ssq[r] = ss;
  __syncthreads();
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = m * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
          const int idx = i * WD_TN + (lane & 31);
          red[idx] = w == 0 ? acc[m][e] : red[idx] + acc[m][e];
        }
    }
    __syncthreads();
  }

  if (KS > 1) {
    // ---- split contraction: store the partial tile, count in; the last arriver sums the splits in order ----
    const int64_t cpad = WD_COUNTERS;
    unsigned* cnt = reinterpret_cast<unsigned*>(work);
    float* parts = work + cpad + (int64_t)tile * KS * B * WD_TN;
    float* sqs = work + cpad + (int64_t)T * KS * B * WD_TN + (int64_t)tile * KS * B;
    for (int idx = tid; idx < B * WD_TN; idx += 256) parts[(int64_t)split * B * WD_TN + idx] = red[idx];
    if (MODE == 1 && tid < B) sqs[split * B + tid] = ss;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // every storing wave
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned old = __hip_atomic_fetch_add(cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int me_last = old == (unsigned)(KS - 1);
      if (me_last) {
        __hip_atomic_store(cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (zero for the next launch)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      last = me_last;
    }
    __syncthreads();
    if (!last) return;
    for (int idx = tid; idx < B * WD_TN; idx += 256) {
      float s = parts[idx];
      for (int sp = 1; sp < KS; ++sp) s += parts[(int64_t)sp * B * WD_TN + idx];
      red[idx] = s;
    }
    if (MODE == 1 && tid < B) {
      float s = sqs[tid];
      for (int sp = 1; sp < KS; ++sp) s += sqs[sp * B + tid];
      ssq[tid] = s;
    }
    __syncthreads();
  }

  // ---- epilogue: the row's RMSNorm scale, bias, store / accumulate, candidates ----
  for (int idx = tid; idx < B * WD_TN; idx += 256) {
    const int i = idx / WD_TN, j = idx - i * WD_TN, nn = n0 + j;
    float v = red[idx];
    if (MODE == 1) v *= 1.f / sqrtf(ssq[i] / (float)K + eps);
    if (nn < N) {
      if (bias) v += bias[nn];
      if (pos == nullptr || pos[i] >= 0) {
        float* yp = y + (int64_t)i * y_rs + nn;
        if (epi == 1) *yp = *yp + v;
        else *yp = v;
      }
    }
    red[idx] = v;
  }
  if (epi == 2) {
    __syncthreads();
    if (tid < B) {                     // first maximum of the tile's columns (ascending), as pdn_decode_gemv_f32 leaves it
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      for (int j = 0; j < WD_TN && n0 + j < N; ++j) {
        const float v = red[tid * WD_TN + j];
        if (v > bv || bi == 0x7fffffff) { bv = v; bi = n0 + j; }
      }
      cand_v[(int64_t)tid * T + tile] = bv;
      cand_i[(int64_t)tid * T + tile] = bi;
    }
  }
}

extern "C" int pdn_decode_wide_blocks(int N) { return N > 0 ? (N + WD_TN - 1) / WD_TN : 0; }

extern "C" int64_t pdn_decode_wide_work_floats(int B, int K, int N) {
  if (B <= 0 || K <= 0 || N <= 0) return 0;
  const int KS = wd_splits(K, N);
  if (KS == 1) return 0;
  const int64_t T = pdn_decode_wide_blocks(N);
  return WD_COUNTERS + T * KS * B * (WD_TN + 1);
}

extern "C" int pdn_decode_wide_supported(int B, int D, int H, int head_dim, int F, int V, int max_len) {
  return B >= 9 && B <= WD_MAX_B && H > 0 && head_dim > 0 && head_dim * H == D && head_dim % 4 == 0 && head_dim <= 256 &&
         D % 4 == 0 && F > 0 && F % 4 == 0 && V > 0 && V <= (1 << 23) && max_len > 0 && max_len * 4 <= 60 * 1024;
}

template <int MT>
static void wide_gemm_go(int mode, dim3 grid, hipStream_t st, const float* x, int64_t x_rs, const float* norm_w, float eps,
                         int ns, int hd, const float* W, int64_t w_rs, int blk_cols, int64_t w_bs, const float* bias,
                         float* y, int64_t y_rs, int epi, float* cand_v, int* cand_i, const int* pos, int B, int K, int N,
                         int per, float* work) {
#define WD_GO(MODE)                                                                                                    \
  hipLaunchKernelGGL((wide_gemm_kernel<MT, MODE>), grid, dim3(256), 0, st, x, x_rs, norm_w, eps, ns, hd, W, w_rs,      \
                     blk_cols, w_bs, bias, y, y_rs, epi, cand_v, cand_i, pos, B, K, N, per, work)
  if (mode == 0) WD_GO(0);
  else if (mode == 1) WD_GO(1);
  else if (mode == 2) WD_GO(2);
  else WD_GO(3);
#undef WD_GO
}

extern "C" int pdn_decode_wide_gemm_f32(const float* x, int64_t x_row_stride, int mode, const float* norm_w, float eps,
                                        int act_ns, int act_hd, const float* W, int64_t w_row_stride, int blk_cols,
                                        int64_t w_block_stride, const float* bias, float* y, int64_t y_row_stride,
                                        int epi, float* cand_v, int* cand_i, const int* pos, int B, int K, int N,
                                        float* work, void* stream) {
  if (B == 0 || N == 0) return PDN_OK;
  PDN_CHECK_ARG(x && W && y && B > 0 && B <= WD_MAX_B && K > 0 && N > 0 && blk_cols > 0 && N % blk_cols == 0 &&
                    mode >= 0 && mode <= 3 && epi >= 0 && epi <= 2,
                "pdn_decode_wide_gemm_f32: bad arguments (B %d, K %d, N %d, mode %d, epi %d)", B, K, N, mode, epi);
  PDN_CHECK_ARG(K % 4 == 0 && x_row_stride % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)norm_w & 15) == 0,
                "pdn_decode_wide_gemm_f32: K and the row stride in multiples of 4, 16-byte aligned rows");
  PDN_CHECK_ARG(w_row_stride >= 0 && w_block_stride >= 0 && y_row_stride >= N, "pdn_decode_wide_gemm_f32: bad strides");
  PDN_CHECK_ARG(mode != 1 || norm_w, "pdn_decode_wide_gemm_f32: mode 1 needs the norm weight");
  PDN_CHECK_ARG(mode != 2 || x_row_stride >= 2 * (int64_t)K, "pdn_decode_wide_gemm_f32: mode 2 rows are [gate | up]");
  PDN_CHECK_ARG(mode != 3 || (act_ns >= 1 && act_ns <= WD_MAX_NS && act_hd > 0 && act_hd % 4 == 0 && K % act_hd == 0 &&
                              x_row_stride >= (int64_t)act_ns * (K / act_hd) * (4 + act_hd)),
                "pdn_decode_wide_gemm_f32: mode 3 needs 1 <= act_ns <= %d partials of head_dim %% 4 == 0", WD_MAX_NS);
  PDN_CHECK_ARG(epi != 2 || (cand_v && cand_i), "pdn_decode_wide_gemm_f32: epi 2 needs cand_v and cand_i");
  const int KS = wd_splits(K, N), per = wd_per(K, N);
  PDN_CHECK_ARG(KS == 1 || work, "pdn_decode_wide_gemm_f32: this shape needs pdn_decode_wide_work_floats(B, K, N) floats "
                                 "of workspace (zeroed once)");
  const dim3 grid(pdn_decode_wide_blocks(N), KS);
  hipStream_t st = (hipStream_t)stream;
  if (B <= 32)
    wide_gemm_go<1>(mode, grid, st, x, x_row_stride, norm_w, eps, act_ns, act_hd, W, w_row_stride, blk_cols, w_block_stride,
                    bias, y, y_row_stride, epi, cand_v, cand_i, pos, B, K, N, per, work);
  else if (B <= 64)
    wide_gemm_go<2>(mode, grid, st, x, x_row_stride, norm_w, eps, act_ns, act_hd, W, w_row_stride, blk_cols, w_block_stride,
                    bias, y, y_row_stride, epi, cand_v, cand_i, pos, B, K, N, per, work);
  else if (B <= 128)
    wide_gemm_go<4>(mode, grid, st, x, x_row_stride, norm_w, eps, act_ns, act_hd, W, w_row_stride, blk_cols, w_block_stride,
                    bias, y, y_row_stride, epi, cand_v, cand_i, pos, B, K, N, per, work);
  else
    wide_gemm_go<8>(mode, grid, st, x, x_row_stride, norm_w, eps, act_ns, act_hd, W, w_row_stride, blk_cols, w_block_stride,
                    bias, y, y_row_stride, epi, cand_v, cand_i, pos, B, K, N, per, work);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_WIDE);
  return PDN_OK;
}

// ---- the wide ticks: one workgroup per row ---------------------------------------------------------------------------
// The step counter is shared by every row: each workgroup reads *step (lane 0, before anything below), then counts in at
// `arrive` with an acquire-release add; the workgroup whose add returns B - 1 knows that every workgroup has read *step,
// and only it writes *step + 1 and puts `arrive` back to 0 for the next launch.  (A plain "row 0 advances it" races with
// workgroups that start later and read the new value; a flag would need a release / acquire pair in every reader.)
__device__ __forceinline__ void wd_count_in(int* step, int* arrive, int p, int B) {
  const int old = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (old == B - 1) {
    __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(step, p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// lane 0 of row b: history slot, the position / budget update of decode_pick_tick_kernel<true, SLOTS> (decode.hip)
template <bool SLOTS>
__device__ __forceinline__ void wd_row_done(int b, int B, int pb, int64_t tok, int* pos, int* step, int* arrive,
                                            const unsigned* stop, int* left, int ring, int64_t* const* hist) {
  const int p = __hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int64_t* hrow = hist ? *hist + (int64_t)(SLOTS ? p % ring : p) * B : nullptr;
  if (pb < 0) {
    if (hrow) __hip_atomic_store(hrow + b, (int64_t)-1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    if (hrow) __hip_atomic_store(hrow + b, tok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (may be host memory)
    const bool hit = stop && ((stop[tok >> 5] >> (tok & 31)) & 1u);
    if (SLOTS) {
      const int lb = left[b] - 1;
      left[b] = lb;
      pos[b] = (lb <= 0 || hit) ? -1 : pb + 1;
    } else {
      pos[b] = hit ? -1 : pb + 1;
    }
  }
  wd_count_in(step, arrive, p, B);
}

template <bool SLOTS>
__global__ __launch_bounds__(256) void wide_pick_tick_kernel(const float* __restrict__ vals, const int* __restrict__ args,
                                                             int B, int n, int64_t* __restrict__ ids, int* pos, int* step,
                                                             int* arrive, const unsigned* __restrict__ stop, int* left,
                                                             int ring, int64_t* const* __restrict__ hist,
                                                             const float* __restrict__ emb, int64_t emb_rs, int D,
                                                             float* __restrict__ x_next) {
  __shared__ float bv[4];
  __shared__ int bi[4];
  __shared__ int64_t chosen;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pb = pos[b];
  if (pb >= 0) {                           // (uniform)
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = tid; i < n; i += 256) {
      const float v = vals[(int64_t)b * n + i];
      const int a = args[(int64_t)b * n + i];
      if (v > best || (v == best && a < idx)) { best = v; idx = a; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(idx, o, 64);
      if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    if (lane == 0) { bv[wave] = best; bi[wave] = idx; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < 4; ++w)
        if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
      chosen = idx == 0x7fffffff ? 0 : idx;
      ids[b] = chosen;
    }
  }
  __syncthreads();                         // (every thread has read pos[b])
  if (tid == 0) wd_row_done<SLOTS>(b, B, pb, pb >= 0 ? chosen : 0, pos, step, arrive, stop, left, ring, hist);
  if (pb >= 0 && emb) {
    const float* row = emb + chosen * emb_rs;
    for (int d = tid; d < D; d += 256) x_next[(int64_t)b * D + d] = row[d];
  }
}

// PER (include/pdn_persample.h): row b uses parameter block prm[b] (a stopped row's is not read), else *prm.
template <bool SLOTS, bool PER>
__global__ __launch_bounds__(SMP_THREADS) void wide_sample_tick_kernel(
    const float* __restrict__ logits, int64_t rs, int B, int V, const SampleParams* __restrict__ prm,
    int64_t* __restrict__ ids, int* pos, int* step, int* arrive, const int* __restrict__ req, int* left, int ring,
    const unsigned* __restrict__ stop, int64_t* const* __restrict__ hist, const float* __restrict__ emb, int64_t emb_rs,
    int D, float* __restrict__ x_next) {
  __shared__ SmpShared s;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int pb = pos[b];
  int64_t tok = 0;
  if (pb >= 0) {                           // (uniform) the draw of sample.hip with counter (pos[b], req[b] or b)
    tok = smp_row<PER>(logits + (int64_t)b * rs, V, prm[PER ? b : 0], (uint64_t)pb, (uint64_t)(SLOTS ? req[b] : b), s);
    if (tid == 0) ids[b] = tok;
  }
  __syncthreads();                         // (every thread has read pos[b])
  if (tid == 0) wd_row_done<SLOTS>(b, B, pb, tok, pos, step, arrive, stop, left, ring, hist);
  if (pb >= 0 && emb) {
    const float* row = emb + tok * emb_rs;
    for (int d = tid; d < D; d += SMP_THREADS) x_next[(int64_t)b * D + d] = row[d];
  }
}

#define WD_TICK_CHECK(name)                                                                                             \
  PDN_CHECK_ARG(ids && pos && step && arrive && B > 0 && B <= WD_MAX_B, name ": bad arguments (B %d)", B);              \
  PDN_CHECK_ARG(!emb || (x_next && D > 0), name ": an embedding table needs x_next and D")

extern "C" int pdn_decode_wide_pick_tick_rows_f32(const float* blk_max, const int* blk_arg, int B, int n_blocks,
                                                  int64_t* ids, int* pos, int* step, int* arrive,
                                                  const unsigned* stop_mask, int64_t* const* history, const float* emb,
                                                  int64_t emb_row_stride, int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  WD_TICK_CHECK("pdn_decode_wide_pick_tick_rows_f32");
  PDN_CHECK_ARG(blk_max && blk_arg && n_blocks > 0, "pdn_decode_wide_pick_tick_rows_f32: bad candidates");
  hipLaunchKernelGGL(wide_pick_tick_kernel<false>, dim3(B), dim3(256), 0, (hipStream_t)stream, blk_max, blk_arg, B,
                     n_blocks, ids, pos, step, arrive, stop_mask, nullptr, 1, history, emb, emb_row_stride, D, x_next);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_WIDE);
  pdn_count(PDN_CNT_DECODE_ROWS);
  return PDN_OK;
}

extern "C" int pdn_decode_wide_pick_tick_slots_f32(const float* blk_max, const int* blk_arg, int B, int n_blocks,
                                                   int64_t* ids, int* pos, int* step, int* arrive, const int* req,
                                                   int* left, int ring, const unsigned* stop_mask,
                                                   int64_t* const* history, const float* emb, int64_t emb_row_stride,
                                                   int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  WD_TICK_CHECK("pdn_decode_wide_pick_tick_slots_f32");
  PDN_CHECK_ARG(blk_max && blk_arg && n_blocks > 0 && left && ring > 0,
                "pdn_decode_wide_pick_tick_slots_f32: bad arguments (ring %d)", ring);
  hipLaunchKernelGGL(wide_pick_tick_kernel<true>, dim3(B), dim3(256), 0, (hipStream_t)stream, blk_max, blk_arg, B,
                     n_blocks, ids, pos, step, arrive, stop_mask, left, ring, history, emb, emb_row_stride, D, x_next);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_WIDE);
  pdn_count(PDN_CNT_DECODE_ROWS);
  pdn_count(PDN_CNT_DECODE_SLOTS);
  return PDN_OK;
}

// PER: the pdnq_ forms of include/pdn_persample.h, `params` = B blocks.
template <bool PER>
static int wide_sample_tick_rows(const char* name, const float* logits, int64_t row_stride, int B, int V,
                                 const void* params, int64_t* ids, int* pos, int* step, int* arrive,
                                 const unsigned* stop_mask, int64_t* const* history, const float* emb,
                                 int64_t emb_row_stride, int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(ids && pos && step && arrive && B > 0 && B <= WD_MAX_B, "%s: bad arguments (B %d)", name, B);
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "%s: an embedding table needs x_next and D", name);
  PDN_CHECK_ARG(logits && params && V > 0 && V <= (1 << 23) && row_stride >= V, "%s: bad logits (V %d)", name, V);
  hipLaunchKernelGGL((wide_sample_tick_kernel<false, PER>), dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits,
                     row_stride, B, V, (const SampleParams*)params, ids, pos, step, arrive, nullptr, nullptr, 1,
                     stop_mask, history, emb, emb_row_stride, D, x_next);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_WIDE);
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_DECODE_ROWS);
  if (PER) pdn_count(PDN_CNT_PERSAMPLE);
  return PDN_OK;
}

template <bool PER>
static int wide_sample_tick_slots(const char* name, const float* logits, int64_t row_stride, int B, int V,
                                  const void* params, int64_t* ids, int* pos, int* step, int* arrive, const int* req,
                                  int* left, int ring, const unsigned* stop_mask, int64_t* const* history,
                                  const float* emb, int64_t emb_row_stride, int D, float* x_next, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(ids && pos && step && arrive && B > 0 && B <= WD_MAX_B, "%s: bad arguments (B %d)", name, B);
  PDN_CHECK_ARG(!emb || (x_next && D > 0), "%s: an embedding table needs x_next and D", name);
  PDN_CHECK_ARG(logits && params && req && left && ring > 0 && V > 0 && V <= (1 << 23) && row_stride >= V,
                "%s: bad arguments (V %d, ring %d)", name, V, ring);
  hipLaunchKernelGGL((wide_sample_tick_kernel<true, PER>), dim3(B), dim3(SMP_THREADS), 0, (hipStream_t)stream, logits,
                     row_stride, B, V, (const SampleParams*)params, ids, pos, step, arrive, req, left, ring, stop_mask,
                     history, emb, emb_row_stride, D, x_next);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_DECODE_WIDE);
  pdn_count(PDN_CNT_SAMPLE);
  pdn_count(PDN_CNT_DECODE_ROWS);
  pdn_count(PDN_CNT_DECODE_SLOTS);
  if (PER) pdn_count(PDN_CNT_PERSAMPLE);
  return PDN_OK;
}

#define WD_SAMPLE_ROWS_ENTRY(name, PER)                                                                                 \
  extern "C" int name(const float* logits, int64_t row_stride, int B, int V, const void* params, int64_t* ids, int* pos, \
                      int* step, int* arrive, const unsigned* stop_mask, int64_t* const* history, const float* emb,     \
                      int64_t emb_row_stride, int D, float* x_next, void* stream) {                                     \
    return wide_sample_tick_rows<PER>(#name, logits, row_stride, B, V, params, ids, pos, step, arrive, stop_mask,       \
                                      history, emb, emb_row_stride, D, x_next, stream);                                 \
  }
#define WD_SAMPLE_SLOTS_ENTRY(name, PER)                                                                                \
  extern "C" int name(const float* logits, int64_t row_stride, int B, int V, const void* params, int64_t* ids, int* pos, \
                      int* step, int* arrive, const int* req, int* left, int ring, const unsigned* stop_mask,           \
                      int64_t* const* history, const float* emb, int64_t emb_row_stride, int D, float* x_next,          \
                      void* stream) {                                                                                   \
    return wide_sample_tick_slots<PER>(#name, logits, row_stride, B, V, params, ids, pos, step, arrive, req, left,      \
                                       ring, stop_mask, history, emb, emb_row_stride, D, x_next, stream);               \
  }
WD_SAMPLE_ROWS_ENTRY(pdn_decode_wide_sample_tick_rows_f32, false)
WD_SAMPLE_ROWS_ENTRY(pdnq_decode_wide_sample_tick_rows_f32, true)
WD_SAMPLE_SLOTS_ENTRY(pdn_decode_wide_sample_tick_slots_f32, false)
WD_SAMPLE_SLOTS_ENTRY(pdnq_decode_wide_sample_tick_slots_f32, true)
