/* Decode attention of a grouped-query model -- the graph-replayed decode step of Llama(n_kv_heads=...): extensions of the
 * pdnhip C ABI (csrc/decode_gqa.hip), exported by libpdnhip.so beside include/pdn_hip.h and bound by pydynet_amd/_lib.py
 * with it.  Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnj_, the joint K/V of a group) of their own: as for include/pdn_gqattn.h and the headers
 * before it -- the tests hold each header, the library's exports under its prefix and the host emulation equal.  This
 * header is listed in _lib.GQDECODE_HEADER_PATHS; the emulation is tests/abi_emulator/_gqdecode.py.
 *
 * Statement: pdn_decode_attention_f32 / pdn_decode_attention_rows_f32 of include/pdn_hip.h for Hkv < H key/value heads (the
 * reference has multi-head attention only: no entry below has a counterpart).  qkv rows, qkv_row_stride floats apart, are
 * [q (H * hd) | k (Hkv * hd) | v (Hkv * hd)]; q and k are rotated by the angle of the row's position (interleaved pairs,
 * cos / sin tables (max_len, hd / 2)); k / v are appended to cache row pos -- cache rows are Hkv * hd floats apart,
 * sequences cache_batch_stride apart; query head h attends to key/value head h / G, G = H / Hkv, over the keys [0, pos].
 * partials: (B, n_splits, H, 4 + hd) floats = [m, l, -, - | sum exp(s - m) v] per (row, key range, QUERY head), the layout
 * of the multi-head entries, so pdn_decode_gemv_f32 (act 2) and pdn_decode_wide_gemm_f32 (mode 3) merge them unchanged; a
 * key range without keys gives [-inf, 0, -, - | zeros].  A workgroup is (row, key/value head, key range) and reads each
 * K / V row once for the G query heads; sums are formed in a fixed order (no atomics: two runs give the same bits).
 * Each launch counts once in launch counter slot 56. */
#ifndef PDN_GQDECODE_H
#define PDN_GQDECODE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1 for a whole group size G = H / Hkv in 2 .. 8, head_dim % 4 == 0, head_dim <= 128, 1 <= n_splits <= 64 and
 * 4 * (G * head_dim + 2 * head_dim + 64 + max(G * roundup4(ceil(max_len / n_splits)), G * (256 / (head_dim / 4)) * head_dim))
 * <= 60 KB of LDS (queries, the new key / value, reductions, then scores | partial sums); else 0 (G = 1 is multi-head
 * attention: pdn_decode_attention_f32). */
int pdnj_decode_attention_supported(int H, int Hkv, int head_dim, int n_splits, int max_len);
/* rows = 0: pos is one int32, every row at position *pos.  rows != 0: pos is (B,), row b at pos[b]; pos[b] < 0 is a
 * stopped row, computed at position 0 with no byte of its cache written.  PDN_EUNSUPPORTED outside
 * pdnj_decode_attention_supported; operands and strides 16-byte aligned, max_len * Hkv * head_dim < 2^31,
 * qkv_row_stride >= (H + 2 Hkv) * head_dim, cache_batch_stride >= max_len * Hkv * head_dim. */
int pdnj_decode_attention_f32(const float* qkv, int64_t qkv_row_stride, const float* cos_table, const float* sin_table,
                              float* k_cache, float* v_cache, float* partials, int B, int H, int Hkv, int head_dim,
                              int n_splits, int64_t cache_batch_stride, const int* pos, int max_len, int rows,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
