/* Document-masked (segmented, "varlen") causal attention for packed training rows: extensions of the pdnhip C ABI
 * (csrc/attention.hip, csrc/segments.hip), exported by libpdnhip.so beside include/pdn_hip.h and bound by
 * pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams, the error flag) are the core header's.
 *
 * Why a header and a prefix (pdns_) of their own: as for include/pdn_optim.h and include/pdn_loss.h -- the tests hold
 * include/pdn_hip.h, the library's pdn_* exports and the closed registry of the host emulation equal.  This header is listed
 * in _lib.SEG_HEADER_PATHS and held to the same three-way equality by tests/test_segattn_abi_cpu.py: the library's pdns_*
 * exports, and the emulation in tests/abi_emulator/_segattn.py with its own NOT_EMULATED.
 *
 * The reference's attention (llm/llama/model.py:112-121) masks by causality alone, so there is no counterpart.
 * Statement: pydynet_amd/core/fused/segments.py.
 *
 *   seg: (B, L) int32, non-decreasing along each row; equal ids = one document (padding at the end of a row is one more)
 *   start[b][i] = smallest j with seg[b][j] == seg[b][i];   end[b][i] = one past the largest such j
 *   query i sees key j  iff  start[b][i] <= j <= i
 *   a key outside that range has probability exactly 0 and receives exactly 0 gradient from that query
 *
 * The bounds live on the device and the host never reads them: a step captured in a hipGraph follows an id buffer whose
 * contents change between replays.  The attention entries run the SEG instantiations of the resident fp32-MFMA kernels
 * (attention_fwd_kernel, attention_bwd_dq_kernel, attention_bwd_dkv_kernel) -- for rotation-free operands too, which
 * without segments go to the persistent kernels.  Key tiles wholly in front of a query tile's document (query tiles wholly
 * behind a key tile's) are not multiplied.  Launch counter slot 43, and 9 / 10 as every resident launch. */
#ifndef PDN_SEGATTN_H
#define PDN_SEGATTN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the segmented kernels take the shape: head_dim 48 / 64, L a multiple of 32 in [32, 1024] (no counterpart) */
int pdns_attention_supported(int L, int head_dim);

/* seg_start / seg_end ((B, L) int32) from seg_ids ((B, L) int32), L <= 4096; one workgroup per row.  A row that decreases
 * somewhere raises *err_flag and gets plain causal bounds: start 0, end L (no counterpart) */
int pdns_segment_bounds_i32(const int* seg_ids, int B, int L, int* seg_start, int* seg_end, int* err_flag, void* stream);

/* pdn_attention_fwd_f32 (always causal) under the document mask; layouts, strides and alignment as there.  rope_cos /
 * rope_sin NULL: the operands are rotation-free or already rotated (no counterpart) */
int pdns_attention_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int L,
                           int head_dim, int64_t row_stride, int64_t batch_stride, int64_t o_row_stride, int64_t o_batch_stride,
                           const float* rope_cos, const float* rope_sin, const int* seg_start, void* stream);

/* pdn_attention_bwd_f32 under the document mask; prerotated != 0: q and k come already rotated and only dq / dk are
 * rotated back as they are stored (pdn_attention_bwd_rotated_f32; the tables are then required).  workspace:
 * pdn_attention_bwd_workspace_bytes(B, H, L) (no counterpart) */
int pdns_attention_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse,
                           float* dq, float* dk, float* dv, int B, int H, int L, int head_dim, int64_t row_stride,
                           int64_t batch_stride, int64_t o_row_stride, int64_t o_batch_stride, const float* rope_cos,
                           const float* rope_sin, int prerotated, const int* seg_start, const int* seg_end, void* workspace,
                           int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
