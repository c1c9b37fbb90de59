// Index arithmetic of the split-fp16 output-resident products C (M x 288) = A (M x K) B (+ bias + residual)
// (csrc/outres_split.hip), shared by the kernels and a host checker (tests/outres_split_check.cpp) that walks every
// workgroup, wave, lane, piece and store step: which global elements a load or a store touches, where a value lies in
// LDS, and the swizzles.  Nothing here depends on HIP.
//
// A PIECE is 32 contraction values.  Its W image (ORS_PIECE = 36 KiB, built once per call by the W pass, copied to LDS as
// it is) has the layout of csrc/lm_head_dx_split.hip: [plane h: 288 columns x 4 units | plane l: the same], a unit = 8
// halves of k, unit q of output column d at ors_img_unit(d, q).
// The row operand A passes through a ring of four 2 KiB pieces private to a wave (sixteen rows x 32 floats).
// The main kernel is PERSISTENT: ors_grid(M) workgroups walk the 128-row blocks b = x, x + grid, ..., as ONE stream of
// (block, piece) pairs -- the fetches that run ahead of the last pieces of a block are the first pieces of the next one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORS_HD __host__ __device__ __forceinline__
#else
#define ORS_HD inline
#endif

#define ORS_N 288                            // output columns: 18 tiles of 16
#define ORS_NT 18
#define ORS_KP 32                            // contraction values per piece = one MFMA k-step
#define ORS_PLANE (ORS_N * ORS_KP * 2)       // bytes of one fp16 plane of a piece
#define ORS_PIECE (2 * ORS_PLANE)            // 36 KiB
#define ORS_RAW 2048                         // a wave's 16 rows x 32 floats of one piece
#define ORS_RING 4                           // pieces of A per wave in LDS
#define ORS_WG_ROWS 128
#define ORS_RING0 (2 * ORS_PIECE)            // two W slots, then eight rings
#define ORS_LDS (ORS_RING0 + 8 * ORS_RING * ORS_RAW)     // 136 KiB (the kernel adds 2 x 1152 bytes: column exponents and bias)
#define ORS_IMG_WGS ((ORS_N * 4 + 255) / 256) // workgroups of 256 threads per piece in the image pass: one unit per thread
#define ORS_DRAIN 6                         // tiles of the residual requested at a time by the drain (18 = 3 groups)
#define ORS_NDRAIN 3                         // tiles of x requested at a time by pass A of the RMSNorm-backward drain (six groups)
#define ORS_MAX_WGS 256                      // one workgroup per CU
#define ORS_MIN_ROWS 65536
#define ORS_MIN_K 256                        // eight pieces: more than the ring holds, so a fetch is never two blocks ahead
#define ORS_MAX_K 4096
#define ORS_NN_LD 289                        // floats per k-row of the transposing pass's LDS tile

ORS_HD int ors_min_i(int a, int b) { return a < b ? a : b; }
ORS_HD int64_t ors_min_l(int64_t a, int64_t b) { return a < b ? a : b; }

// ---- the grid ----------------------------------------------------------------------------------------------------------
ORS_HD int ors_blocks(int64_t M) { return (int)((M + ORS_WG_ROWS - 1) / ORS_WG_ROWS); }
ORS_HD int ors_grid(int64_t M) { return ors_min_i(ors_blocks(M), ORS_MAX_WGS); }
// the block behind `blk` of a workgroup of a grid of `grid`; `blk` itself behind the last (its fetches are then repeated)
ORS_HD int ors_next_block(int blk, int grid, int nblk) { return blk + grid < nblk ? blk + grid : blk; }

// ---- W ---------------------------------------------------------------------------------------------------------------
// byte offset, inside a plane, of unit q (k = 8 q .. 8 q + 7 of the piece) of output column d: the sixteen columns x four
// units one ds_read_b128 fetches cover every 16-byte slot of the banks four times
ORS_HD int ors_img_unit(int d, int q) { return (d * 4 + (q ^ ((d >> 2) & 3))) * 16; }
// lane (r, q) of a wave reads, for tile j, unit q of column 16 j + r: ors_frag(r, q) + 1024 j
ORS_HD int ors_frag(int r, int q) { return ors_img_unit(r, q); }
// NT (B = W (288 x K) as stored, or nb blocks (288 x kb) `bstride` floats apart, ppb = kb / 32 pieces each): float offset
// from block 0 of the eight values k = 8 q .. + 7 of piece `piece`, column d; ldb = floats between two rows of a block
ORS_HD int64_t ors_w_src_nt(int piece, int d, int q, int ppb, int64_t ldb, int64_t bstride) {
  const int b = piece / ppb;
  return (int64_t)b * bstride + (int64_t)d * ldb + (int64_t)(piece - b * ppb) * ORS_KP + 8 * q;
}
// NN (B (K x 288) row-major): the transposing pass reads float4 i (0 .. 2303) of a piece, row k = i / 72 of the piece,
// columns 4 (i % 72) .. + 3 -- whole 1152-byte rows, coalesced -- into an LDS tile, element (k, d) at ors_nn_lds(k, d)
ORS_HD int64_t ors_w_src_nn(int piece, int i, int64_t ldb) { return ((int64_t)piece * ORS_KP + i / 72) * ldb + 4 * (i % 72); }
ORS_HD int ors_nn_lds(int k, int d) { return k * ORS_NN_LD + d; }
// DMA instruction e (0..4) of wave w copies bytes 1024 I .. + 1023 of an image, I = ors_wdma_instr(e, w) (the last four
// waves repeat instruction 35, so that every wave counts the same memory operations)
ORS_HD int ors_wdma_instr(int e, int wave) { return ors_min_i(e * 8 + wave, 35); }

// ---- A -----------------------------------------------------------------------------------------------------------------
// DMA instruction i (0, 1) of a piece: lane l fetches, for row ors_raw_row(i, l) of the wave's sixteen, the 16-byte chunk
// ors_raw_chunk(i, l) of the row's 128 bytes, which lands at ring byte 1024 i + 16 l
ORS_HD int ors_raw_row(int i, int lane) { return 8 * i + (lane >> 3); }
ORS_HD int ors_raw_chunk(int i, int lane) { return (lane & 7) ^ ((ors_raw_row(i, lane) >> 1) & 7); }
// the row of A behind row rr of wave `wave` of block `blk` (rows past the end: the last row, nothing stored)
ORS_HD int64_t ors_a_row(int blk, int wave, int rr, int64_t M) { return ors_min_l((int64_t)blk * ORS_WG_ROWS + wave * 16 + rr, M - 1); }
// lane (r, q) reads the floats 8 q .. 8 q + 7 of row r: chunk 2 q at ors_raw_lane(r, q), chunk 2 q + 1 at that ^ 16
ORS_HD int ors_raw_lane(int r, int q) { return r * 128 + (((2 * q) ^ ((r >> 1) & 7)) << 4); }
// the piece whose fetch is issued while piece s of a block of np runs, and whether it belongs to the NEXT block
ORS_HD int ors_ahead_piece(int s, int np) { return s + ORS_RING < np ? s + ORS_RING : s + ORS_RING - np; }
ORS_HD bool ors_ahead_next(int s, int np) { return s + ORS_RING >= np; }

// ---- C: lane (r, q) stores columns 16 j + 4 q .. + 3 of row r for tile j ---------------------------------------------------
ORS_HD int ors_out_col(int j, int q) { return 16 * j + 4 * q; }

// ---- the RMSNorm-backward drain (epilogue 1): lane (r, q) of wave w owns row ors_lane_row(blk, w, r) and, for tile j, its
// columns ors_out_col(j, q) .. + 3, of x, of the held gradient and of dx alike; a row >= M reads x and rms of the last row
// (ors_min_l(row, M - 1), as ors_a_row does for A), adds zeros to the weight-gradient sums and stores nothing.
// The weight-gradient sums of a wave's sixteen rows go into a row of LDS private to the wave, float ors_dw_lds(w, col)
// of ORS_DW_FLOATS (behind the 288 norm weights in the same array); the r == 0 lanes add there, columns ors_out_col(j, q).
#define ORS_DW_FLOATS (8 * ORS_N)
#define ORS_NORM_FLOATS (ORS_N + ORS_DW_FLOATS)   // the epilogue's LDS: [288 weights | 8 waves x 288 sums]
ORS_HD int64_t ors_lane_row(int blk, int wave, int r) { return (int64_t)blk * ORS_WG_ROWS + wave * 16 + r; }
ORS_HD int ors_dw_lds(int wave, int col) { return wave * ORS_N + col; }

// ---- the running exponent of a row --------------------------------------------------------------------------------------
#define ORS_UNSET (1 << 20)                  // no finite non-zero value seen yet: every maximum moves it
// E = the frexp exponent of the largest finite magnitude `mx` of the row's next 32 values (mx in [2^(E-1), 2^E)); S the
// exponent so far.  mx 2^S would reach 2^15: S such that mx lands in [2^12, 2^13).  S only falls; mx == 0 is ignored.
ORS_HD int ors_next_exp(bool nonzero, int E, int S) { return (nonzero && E + S >= 16) ? 13 - E : S; }
