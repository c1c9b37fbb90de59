// Token-FSM constrained decoding of a decode step (Llama.generate / generate_ragged / serve with token_fsm); the contract is
// stated in NumPy in llm/token_fsm.py, the ABI in include/pdn_fsm.h.  The machines of a call are CSR tables the kernels
// only read: offsets (S + 1), tokens (E, ascending within a state), next (E), dflt (S).  Row state, per plan: state (B,)
// int64, the word (position << 32) | state -- the state the row is in at that position; start_state (B,), the state of a
// row that has generated nothing; start (B,), the position of the row's first generated token (its prompt length).
//
//   fsm_reset_kernel  one thread per listed row: its start state, prompt length and word.
//   fsm_kernel        grid (chunks, B): a vocabulary chunk of 1024 tokens per workgroup, 4 consecutive tokens per thread
//                     (one 16-byte load and store where the rows' addresses allow it).  Every workgroup of a row works
//                     out the row's state for itself (below); a state without a default then has each thread find the
//                     place of its first token among the state's sorted tokens by binary search and compare its 4 tokens
//                     with the 4 entries from there on.  A state with a default allows everything: its rows are not
//                     stored.  The chunk's first maximum and its index go to cand_v / cand_i (B, chunks): the layout the
//                     pick ticks reduce.
// The state hand-off: all chunk workgroups of a row need the advanced state, exactly one may store it, and nothing orders
// workgroups of one launch.  So each derives it from what it reads -- the word is read with ONE 8-byte load and stored,
// by the workgroup of chunk 0 alone, with ONE 8-byte store: a reader sees either the old word (a position before this
// one: it advances the state by the fed token, one binary search) or the new one (this position: taken as it is), and
// both give the same state.  No atomics, and no search of a bit set built with them: a thread looks its tokens up itself.
// A row at position < 0 (stopped / empty) is left untouched, its word too.
#include "common.h"

#define FS_THREADS 256
#define FS_PER 4
#define FS_CHUNK (FS_THREADS * FS_PER)   // 1024 tokens

extern "C" int pdnf_fsm_chunks(int V) { return V > 0 ? (V + FS_CHUNK - 1) / FS_CHUNK : 0; }

__global__ __launch_bounds__(FS_THREADS) void fsm_reset_kernel(
    long long* __restrict__ state, int* __restrict__ start_state, int* __restrict__ start, int B,
    const int* __restrict__ rows, int n_rows, const int* __restrict__ src_state, const int* __restrict__ src_start) {
  const int i = blockIdx.x * FS_THREADS + threadIdx.x;
  if (i >= n_rows) return;
  const int b = rows[i];
  if (b < 0 || b >= B) return;
  const int s = src_state[i], p = src_start[i];
  start_state[b] = s;
  start[b] = p;
  state[b] = ((long long)p << 32) | (long long)(unsigned)s;
}

// the first j in [lo, hi) with t[j] >= v (hi when there is none)
__device__ __forceinline__ int fs_lower_bound(const int* __restrict__ t, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the edges of state s, [lo, hi), inside [0, E) whatever the table holds
__device__ __forceinline__ void fs_edges(const int* __restrict__ offsets, int E, int s, int& lo, int& hi) {
  lo = min(max(offsets[s], 0), E);
  hi = min(max(offsets[s + 1], lo), E);
}

// STEP: the plan's form -- the state from the row's word, start state and prompt length (sv = start_state), the word stored
// by chunk 0; else the state is sv[b], read only, and pos may be null.
template <bool STEP, bool VEC>
__global__ __launch_bounds__(FS_THREADS) void fsm_kernel(
    float* __restrict__ logits, int64_t rs, int V, const int* __restrict__ offsets, const int* __restrict__ tokens,
    const int* __restrict__ next, const int* __restrict__ dflt, int S, int E, long long* state,
    const int* __restrict__ sv, const int* __restrict__ start, const long long* __restrict__ ids,
    const int* __restrict__ pos, int pos_rows, float* __restrict__ cand_v, int* __restrict__ cand_i) {
  __shared__ float wv[FS_THREADS / 64];
  __shared__ int wi[FS_THREADS / 64];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = c * FS_CHUNK;
  float* z = logits + (int64_t)b * rs;
  const int v0 = c0 + tid * FS_PER;
  const bool in = v0 < V;
  const int vs = in ? v0 : c0;                   // (c0 < V: the grid has ceil(V / 1024) chunks)
  float x[FS_PER];
  if constexpr (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(z + vs);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int u = 0; u < FS_PER; ++u) x[u] = z[min(vs + u, V - 1)];
  }
  const int p = pos ? pos[pos_rows ? b : 0] : 0;
  int cur;
  if constexpr (STEP) {
    const long long w = *reinterpret_cast<const volatile long long*>(state + b);     // one 8-byte load
    const int s0 = sv[b], p0 = start[b];
    const long long t64 = ids[b];
    if (p < 0) return;                           // (uniform) a row that computes nothing: untouched
    cur = (int)(unsigned)(w & 0xffffffffll);
    if (p - p0 <= 0) {
      cur = s0;
    } else if ((int)(w >> 32) != p && cur >= 0 && cur < S) {
      const int tok = (t64 < 0 || t64 > 0x7fffffffll) ? -1 : (int)t64;              // (no edge has a negative token)
      int lo, hi;
      fs_edges(offsets, E, cur, lo, hi);
      const int d = dflt[cur];
      const int j = fs_lower_bound(tokens, lo, hi, tok);
      if (j < hi && tokens[j] == tok) cur = next[j];
      else if (d >= 0) cur = d;
    }
    if (c == 0 && tid == 0) state[b] = ((long long)p << 32) | (long long)(unsigned)cur;   // one 8-byte store
  } else {
    cur = sv[b];
    if (p < 0) return;                           // (uniform)
  }
  bool all = cur < 0 || cur >= S;                // (off, or no state of the tables: no mask)
  int lo = 0, hi = 0;
  if (!all) {
    if (dflt[cur] >= 0) all = true;
    else fs_edges(offsets, E, cur, lo, hi);
  }
  if (all && !cand_v) return;                    // (uniform) nothing to mask, nothing to reduce
  float best = -INFINITY;
  int idx = 0x7fffffff;
  if (in) {
    int t[FS_PER];
    if (!all) {
      const int j = fs_lower_bound(tokens, lo, hi, v0);
#pragma unroll
      for (int u = 0; u < FS_PER; ++u) t[u] = j + u < hi ? tokens[j + u] : -1;
    }
    // (the state's tokens ascend without repeats: the 4 entries from j on hold every token of v0 .. v0 + 3 it has)
#pragma unroll
    for (int u = 0; u < FS_PER; ++u) {
      const int v = v0 + u;
      if (v < V) {
        float xx = x[u];
        if (!all) {
          bool ok = false;
#pragma unroll
          for (int q = 0; q < FS_PER; ++q) ok = ok || t[q] == v;
          if (!ok) xx = -INFINITY;
        }
        x[u] = xx;
        if (xx > best || (xx == best && v < idx)) { best = xx; idx = v; }     // (ascending v: the first maximum; NaN never)
      }
    }
    if (!all) {
      if constexpr (VEC) {
        *reinterpret_cast<float4*>(z + v0) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
#pragma unroll
        for (int u = 0; u < FS_PER; ++u)
          if (v0 + u < V) z[v0 + u] = x[u];
      }
    }
  }
  if (!cand_v) return;                           // (uniform)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
  }
  if (lane == 0) { wv[wave] = best; wi[wave] = idx; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < FS_THREADS / 64; ++w)
      if (wv[w] > best || (wv[w] == best && wi[w] < idx)) { best = wv[w]; idx = wi[w]; }
    if (idx == 0x7fffffff) {                     // nothing but NaN in the chunk: numpy.argmax's answer, its first token
      best = __int_as_float(0x7fc00000);
      idx = c0;
    }
    const int64_t o = (int64_t)b * gridDim.x + c;
    cand_v[o] = best;
    cand_i[o] = idx;
  }
}

// every group of 4 tokens of every row 16-byte aligned and whole
static bool fs_vec(const float* logits, int64_t rs, int V) {
  return ((uintptr_t)logits & 15) == 0 && rs % 4 == 0 && V % 4 == 0;
}

extern "C" int pdnf_fsm_reset(int64_t* state, int* start_state, int* start, int B, const int* rows, int n_rows,
                              const int* src_state, const int* src_start, void* stream) {
  if (n_rows == 0) return PDN_OK;
  PDN_CHECK_ARG(state && start_state && start && rows && src_state && src_start && B > 0 && n_rows > 0 &&
                    ((uintptr_t)state & 7) == 0,
                "pdnf_fsm_reset: bad arguments (B %d, rows %d)", B, n_rows);
  hipLaunchKernelGGL(fsm_reset_kernel, dim3((n_rows + FS_THREADS - 1) / FS_THREADS), dim3(FS_THREADS), 0,
                     (hipStream_t)stream, (long long*)state, start_state, start, B, rows, n_rows, src_state, src_start);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_TOKEN_FSM);
  return PDN_OK;
}

extern "C" int pdnf_fsm_step_f32(float* logits, int64_t row_stride, int B, int V, const int* offsets, const int* tokens,
                                 const int* next, const int* dflt, int S, int E, int64_t* state, const int* start_state,
                                 const int* start, const int64_t* ids, const int* pos, int pos_per_row, float* cand_v,
                                 int* cand_i, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && offsets && tokens && next && dflt && state && start_state && start && ids && pos && B > 0 &&
                    B <= 65535 && V > 0 && S > 0 && E > 0 && row_stride >= V && (!cand_v == !cand_i) &&
                    ((uintptr_t)state & 7) == 0,
                "pdnf_fsm_step_f32: bad arguments (B %d, V %d, S %d, E %d, row stride %lld)", B, V, S, E,
                (long long)row_stride);
  const dim3 grid(pdnf_fsm_chunks(V), B);
  if (fs_vec(logits, row_stride, V))
    hipLaunchKernelGGL((fsm_kernel<true, true>), grid, dim3(FS_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                       offsets, tokens, next, dflt, S, E, (long long*)state, start_state, start, (const long long*)ids,
                       pos, pos_per_row, cand_v, cand_i);
  else
    hipLaunchKernelGGL((fsm_kernel<true, false>), grid, dim3(FS_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                       offsets, tokens, next, dflt, S, E, (long long*)state, start_state, start, (const long long*)ids,
                       pos, pos_per_row, cand_v, cand_i);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_TOKEN_FSM);
  return PDN_OK;
}

extern "C" int pdnf_fsm_rows_f32(float* logits, int64_t row_stride, int B, int V, const int* offsets, const int* tokens,
                                 const int* dflt, int S, int E, const int* states, const int* pos, float* cand_v,
                                 int* cand_i, void* stream) {
  if (B == 0) return PDN_OK;
  PDN_CHECK_ARG(logits && offsets && tokens && dflt && states && B > 0 && B <= 65535 && V > 0 && S > 0 && E > 0 &&
                    row_stride >= V && (!cand_v == !cand_i),
                "pdnf_fsm_rows_f32: bad arguments (B %d, V %d, S %d, E %d, row stride %lld)", B, V, S, E,
                (long long)row_stride);
  const dim3 grid(pdnf_fsm_chunks(V), B);
  if (fs_vec(logits, row_stride, V))
    hipLaunchKernelGGL((fsm_kernel<false, true>), grid, dim3(FS_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                       offsets, tokens, (const int*)nullptr, dflt, S, E, (long long*)nullptr, states, (const int*)nullptr,
                       (const long long*)nullptr, pos, 1, cand_v, cand_i);
  else
    hipLaunchKernelGGL((fsm_kernel<false, false>), grid, dim3(FS_THREADS), 0, (hipStream_t)stream, logits, row_stride, V,
                       offsets, tokens, (const int*)nullptr, dflt, S, E, (long long*)nullptr, states, (const int*)nullptr,
                       (const long long*)nullptr, pos, 1, cand_v, cand_i);
  PDN_LAUNCH_CHECK();
  pdn_count(PDN_CNT_TOKEN_FSM);
  return PDN_OK;
}
