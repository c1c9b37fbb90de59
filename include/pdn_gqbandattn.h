/* Sliding-window attention over grouped heads -- fused.attention(..., window=W) with fewer key/value heads than query heads,
 * Llama(n_kv_heads=..., sliding_window=...): extensions of the pdnhip C ABI (csrc/attention_gqband.hip), exported by
 * libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes,
 * pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnm_, the Mistral layer) of their own: as for include/pdn_bandattn.h and the headers before
 * it -- the tests hold each header and the library's exports under its prefix equal.  This header is listed in
 * _lib.GQBAND_HEADER_PATHS.  There is no host emulation: under the emulator fused.attention runs a window as an additive
 * mask on the paths it has.
 *
 * Statement: pydynet_amd/core/fused/band.py over pydynet_amd/core/fused/gqa.py (the reference has plain causal multi-head
 * attention only: no entry below has a counterpart).  q, o, dq, d_o: (B, Lq, H, hd) through (q_row_stride,
 * q_batch_stride); k, v, dk, dv: (B, Lk, Hkv, hd) through the kv strides; lse: (B, H, Lq).  Query i of head h sits at
 * absolute position i + start_pos and sees the keys max(0, i + start_pos - window + 1) .. i + start_pos of key/value head
 * h / (H / Hkv); there is no mask operand, and K / V are never expanded.  A key outside the band has probability exactly 0
 * and receives exactly 0 gradient from that query; rows of dk / dv no query sees are written as zeros.  dk / dv sum the
 * group in accumulator registers in a fixed order (no atomics, no workspace of expanded gradients; two runs give the same
 * bits).  window >= start_pos + Lq is plain causal grouped-query attention.  Operands and strides 16-byte aligned, heads
 * packed (stride hd).  Each launching entry counts once in launch counter slot 59. */
#ifndef PDN_GQBANDATTN_H
#define PDN_GQBANDATTN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1 for head_dim in {16, 24, 32, 48, 64, 96, 128} and H = G * Hkv with G in 2 .. 8; else 0.  No counterpart. */
int pdnm_attention_supported(int head_dim, int H, int Hkv);
/* B * Hkv <= 65535 (the grid's y extent); any Lq > 0, Lk >= start_pos + Lq.  PDN_EUNSUPPORTED outside
 * pdnm_attention_supported, for window < 1 or for Lk < start_pos + Lq; arguments are checked before the launch.
 * No counterpart. */
int pdnm_attention_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int Hkv,
                           int Lq, int Lk, int head_dim, int64_t q_row_stride, int64_t q_batch_stride,
                           int64_t kv_row_stride, int64_t kv_batch_stride, int start_pos, int window, void* stream);
/* The workspace of pdnm_attention_bwd_f32: delta = rowsum(dO * O), (B, H, Lq) floats.  No counterpart. */
int64_t pdnm_attention_bwd_workspace_bytes(int B, int H, int Lq);
/* Two launches: dQ (which also writes delta), then dK / dV.  Status as the forward entry's; PDN_EWORKSPACE for a short
 * workspace.  No counterpart. */
int pdnm_attention_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                           const float* lse, float* dq, float* dk, float* dv, int B, int H, int Hkv, int Lq, int Lk,
                           int head_dim, int64_t q_row_stride, int64_t q_batch_stride, int64_t kv_row_stride,
                           int64_t kv_batch_stride, int start_pos, int window, void* workspace, int64_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
