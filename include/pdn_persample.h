/* Sampling parameters per row -- temperature, top_k, top_p, min_p and seed of each request of a batch: extensions of the
 * pdnhip C ABI (csrc/sample.hip, csrc/decode_wide.hip, csrc/speculative.hip), exported by libpdnhip.so beside
 * include/pdn_hip.h and bound by pydynet_amd/_lib.py with it.  Conventions (status codes, pdn_last_error, streams) are the
 * core header's.
 *
 * Why a header and a prefix (pdnq_) of their own: as for include/pdn_optim.h, include/pdn_loss.h, include/pdn_segattn.h,
 * include/pdn_rowloss.h, include/pdn_smoothloss.h and include/pdn_logitedit.h -- the tests hold each header, the library's
 * exports under its prefix and the closed registry of the host emulation equal.  This header is listed in
 * _lib.PERSAMPLE_HEADER_PATHS and held to the same three-way equality by tests/test_persample_abi_cpu.py: the library's
 * pdnq_* exports, and the emulation in tests/abi_emulator/_persample.py with its own NOT_EMULATED.
 *
 * Statement: pydynet_amd/llm/sampling.py (the reference's generation, llm/llama/model.py:258-269, takes the argmax: no
 * entry below has a counterpart).  Every entry is the shared-parameter entry of include/pdn_hip.h named after it with one
 * difference: `params` points at B blocks of pdn_sample_params (24 bytes each, a DEVICE pointer) and row b is drawn with
 * block b -- the same device function on the same logits and counter, so a row whose block (min_p = 0) equals the shared
 * block yields the shared entry's token bit for bit.  A row at a position < 0 is left alone and its block is not read.
 *   temperature <= 0  the row yields the first maximum of its logits;
 *   min_p             the float at offset 12 of the block (the former padding; 0 = off, in [0, 1)): after top-k and top-p,
 *                     a kept token stays kept iff exp((z_i - max z) / T) >= min_p; the maximum always stays.  In the
 *                     kernel's integer mass units: weights below (uint64)(min_p * 2^40) leave the draw.  Only the
 *                     entries of this header read it: the shared-parameter entries are the sampler of before (their
 *                     callers write 0 there).
 * Nothing is allocated or read back inside a call, the blocks are only read: a step that ends in one of the ticks replays
 * from a hipGraph while the host rewrites blocks between replays.  Each entry counts once in launch counter slot 49 and
 * wherever its shared-parameter form counts. */
#ifndef PDN_PERSAMPLE_H
#define PDN_PERSAMPLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* pdn_sample_rows_f32 with, per row, a block, a position and a counter id: row b with pos[b] >= 0 is drawn with counter
 * (pos[b], req[b]) (req NULL: (pos[b], b)) into out_ids[b]; nothing else is written, pos is only read.  B <= 65535, one
 * workgroup per row (no counterpart). */
int pdnq_sample_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params, const int* pos,
                         const int* req, int64_t* out_ids, void* stream);
/* pdn_decode_sample_tick_rows_f32 / pdn_decode_sample_tick_slots_f32 (one workgroup walks the B rows) with block b for row
 * b, read by every thread before the first barrier of the row's draw (no counterpart). */
int pdnq_decode_sample_tick_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                     int64_t* next_ids, int* pos, int* step, const unsigned* stop_mask,
                                     int64_t* const* history, const float* emb, int64_t emb_row_stride, int D, float* x_next,
                                     void* stream);
int pdnq_decode_sample_tick_slots_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                      int64_t* next_ids, int* pos, int* step, const int* req, int* left, int ring,
                                      const unsigned* stop_mask, int64_t* const* history, const float* emb,
                                      int64_t emb_row_stride, int D, float* x_next, void* stream);
/* pdn_decode_wide_sample_tick_rows_f32 / pdn_decode_wide_sample_tick_slots_f32 (a workgroup per row, 9 .. 256 rows) with
 * block b for row b (no counterpart). */
int pdnq_decode_wide_sample_tick_rows_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                          int64_t* next_ids, int* pos, int* step, int* arrive, const unsigned* stop_mask,
                                          int64_t* const* history, const float* emb, int64_t emb_row_stride, int D,
                                          float* x_next, void* stream);
int pdnq_decode_wide_sample_tick_slots_f32(const float* logits, int64_t row_stride, int B, int V, const void* params,
                                           int64_t* next_ids, int* pos, int* step, int* arrive, const int* req, int* left,
                                           int ring, const unsigned* stop_mask, int64_t* const* history, const float* emb,
                                           int64_t emb_row_stride, int D, float* x_next, void* stream);
/* pdn_spec_verify_sample_tick_f32 with block r / (k + 1) for query row r: the block of the row it verifies
 * (no counterpart). */
int pdnq_spec_verify_sample_tick_f32(const float* logits, int64_t row_stride, int V, const void* params,
                                     const int64_t* tokens, const int* qpos, int B, int k, int64_t* picks, int* hist,
                                     int hist_stride, int* hist_len, int* pos, int* left, const int* stop_mask, int* step,
                                     int64_t* const* mailbox, void* stream);

#ifdef __cplusplus
}
#endif
#endif
