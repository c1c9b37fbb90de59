/* Decode attention of a sliding-window model -- the graph-replayed decode step of Llama(sliding_window=...), with or without
 * grouped heads: extensions of the pdnhip C ABI (csrc/decode_band.hip), exported by libpdnhip.so beside include/pdn_hip.h
 * and bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams) are the core header's.
 *
 * Why a header and a prefix (pdnv_, the view a row has of its cache) of their own: as for include/pdn_gqdecode.h and the
 * headers before it -- the tests hold each header, the library's exports under its prefix and the host emulation equal.
 * This header is listed in _lib.BANDDECODE_HEADER_PATHS; the emulation is tests/abi_emulator/_banddecode.py.
 *
 * Statement: pdnj_decode_attention_f32 of include/pdn_gqdecode.h with one change -- row b at position p attends to the keys
 * lo .. p, lo = max(0, p - window + 1), not 0 .. p (the reference has neither a window nor grouped heads: no entry below has
 * a counterpart).  qkv rows, qkv_row_stride floats apart, are [q (H * hd) | k (Hkv * hd) | v (Hkv * hd)]; q and k are rotated
 * by the angle of the row's position (interleaved pairs, cos / sin tables (max_len, hd / 2)); k / v are appended to LINEAR
 * cache row pos -- cache rows are Hkv * hd floats apart, sequences cache_batch_stride apart; query head h attends to
 * key/value head h / G, G = H / Hkv in 1 .. 8 (G = 1: a windowed multi-head model).  A cache row outside [lo, p] is
 * neither read nor written.
 * partials: (B, n_splits, H, 4 + hd) floats = [m, l, -, - | sum exp(s - m) v] per (row, key range, QUERY head), the layout
 * of the multi-head entries, so pdn_decode_gemv_f32 (act 2) and pdn_decode_wide_gemm_f32 (mode 3) merge them unchanged; a
 * key range without keys gives [-inf, 0, -, - | zeros].  The ranges cut the window, not the cache: with n = p - lo + 1 keys,
 * range sp holds the keys lo + sp * ceil(n / n_splits) up to the next range's first (the last non-empty one ends at p and
 * owns the new key).  A workgroup is (row, key/value head, key range) and reads each K / V row once for the G query heads;
 * sums are formed in a fixed order (no atomics: two runs give the same bits).  window >= max_len is plain causal decode
 * attention.  Each launch counts once in launch counter slot 58. */
#ifndef PDN_BANDDECODE_H
#define PDN_BANDDECODE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 1 for a whole group size G = H / Hkv in 1 .. 8, head_dim % 4 == 0, head_dim <= 128, 1 <= n_splits <= 64, window >= 1,
 * max_len >= 1 and, with chunk = ceil(min(window, max_len) / n_splits),
 * 4 * (G * head_dim + 2 * head_dim + 64 + max(G * roundup4(chunk), G * (256 / (head_dim / 4)) * head_dim)) <= 60 KB of LDS
 * (queries, the new key / value, reductions, then scores | partial sums); else 0.  The bound follows the window: a long
 * cache with a short window passes it. */
int pdnv_decode_attention_supported(int H, int Hkv, int head_dim, int n_splits, int window, int max_len);
/* rows = 0: pos is one int32, every row at position *pos.  rows != 0: pos is (B,), row b at pos[b]; pos[b] < 0 is a
 * stopped row, computed at position 0 with no byte of its cache written.  PDN_EUNSUPPORTED outside
 * pdnv_decode_attention_supported; operands and strides 16-byte aligned, max_len * Hkv * head_dim < 2^31,
 * qkv_row_stride >= (H + 2 Hkv) * head_dim, cache_batch_stride >= max_len * Hkv * head_dim. */
int pdnv_decode_attention_f32(const float* qkv, int64_t qkv_row_stride, const float* cos_table, const float* sin_table,
                              float* k_cache, float* v_cache, float* partials, int B, int H, int Hkv, int head_dim,
                              int n_splits, int64_t cache_batch_stride, const int* pos, int max_len, int window, int rows,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
