/* Grouped-query attention -- fused.attention with fewer key/value heads than query heads, Llama(n_kv_heads=...):
 * extensions of the pdnhip C ABI (csrc/attention_gqa.hip), exported by libpdnhip.so beside include/pdn_hip.h and bound by
 * pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnk_, the shared K/V) of their own: as for include/pdn_dropout.h and the headers before it --
 * the tests hold each header, the library's exports under its prefix and the host emulation equal.  This header is listed
 * in _lib.GQA_HEADER_PATHS; the emulation is tests/abi_emulator/_gqa.py.  (pdng_ is taken: include/pdn_normgrad.h.)
 *
 * Statement: pydynet_amd/core/fused/gqa.py (the reference has multi-head attention only: no entry below has a
 * counterpart).  q, o, dq, d_o: (B, Lq, H, hd) through (q_row_stride, q_batch_stride); k, v, dk, dv: (B, Lk, Hkv, hd)
 * through the kv strides, H = G * Hkv; query head h reads key/value head h / G.  lse: (B, H, Lq).  o, dq and lse are what
 * pdn_attention_stream_* give on K/V repeated G times along the head axis; dk / dv of head j are the sums of the expanded
 * gradients over heads j * G .. j * G + G - 1 -- formed in accumulator registers in a fixed order (no atomics, no expanded
 * tensor in memory; two runs give the same bits).  causal: key > query + start_pos masked.  mask: additive, element
 * (b, h, q, k) at b*mask_sb + h*mask_sh + q*mask_sq + k*mask_sk with h the QUERY head (0 strides broadcast), NULL = none.
 * Operands and strides 16-byte aligned, heads packed (stride hd).  Each launching entry counts once in launch counter
 * slot 55. */
#ifndef PDN_GQATTN_H
#define PDN_GQATTN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1 for head_dim in {16, 24, 32, 48, 64, 96, 128} and a whole group size G = H / Hkv in 2 .. 8; else 0 (G = 1 is
 * multi-head attention: pdn_attention_* / pdn_attention_stream_*). */
int pdnk_attention_supported(int head_dim, int H, int Hkv);
/* B * Hkv <= 65535 (the grid's y extent); any Lq, Lk > 0. */
int pdnk_attention_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, int B, int H, int Hkv,
                           int Lq, int Lk, int head_dim, int64_t q_row_stride, int64_t q_batch_stride,
                           int64_t kv_row_stride, int64_t kv_batch_stride, int causal, int start_pos,
                           const float* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int64_t mask_sk,
                           void* stream);
/* The workspace of pdnk_attention_bwd_f32: delta = rowsum(dO * O), (B, H, Lq) floats. */
int64_t pdnk_attention_bwd_workspace_bytes(int B, int H, int Lq);
/* Two launches: dQ (which also writes delta), then dK / dV.  PDN_EWORKSPACE for a short workspace. */
int pdnk_attention_bwd_f32(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                           const float* lse, float* dq, float* dk, float* dv, int B, int H, int Hkv, int Lq, int Lk,
                           int head_dim, int64_t q_row_stride, int64_t q_batch_stride, int64_t kv_row_stride,
                           int64_t kv_batch_stride, int causal, int start_pos, const float* mask, int64_t mask_sb,
                           int64_t mask_sh, int64_t mask_sq, int64_t mask_sk, void* workspace, int64_t workspace_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif
