// Index arithmetic of the split-fp16 packed layer weight gradients (csrc/outres_tn_split.hip), shared by the kernels and a
// host checker (tests/outres_tn_split_check.cpp) that walks every workgroup, wave, lane and piece: which global bytes a DMA
// or a store touches, where they land in LDS, and the swizzles.  Nothing here depends on HIP.  The piece, the unit and the
// fragment of an x image and the swizzle of the raw ring are those of the lm_head weight gradient
// (csrc/lm_head_dw_split_index.h); what differs:
//   X image of a piece (OTS_XPIECE = 36 KiB): [plane h: 288 x 4 units | plane l: 288 x 4 units], no tail;
//   g of a piece for a workgroup's 128 columns: 32 rows x 512 bytes in a ring of four, rows `ldg` floats apart in memory
//     (ldg >= n_all: the matrix may be padded), columns past n_all clamped to the row's last 16 bytes;
//   output: block b = column / nb_cols of K range s at C + b * blk_stride + s * slab, rows of nb_cols floats (the batched
//     layout of gemm_splitk_reduce_kernel).
#pragma once
#include "lm_head_dw_split_index.h"

#define OTS_XDMA 36                                 // DMA instructions (1 KiB each) per image
#define OTS_XPIECE (OTS_XDMA * 1024)                // 36 KiB = 2 * LDW_PLANE
#define OTS_COLS LDW_COLS                           // 128 columns per workgroup: 8 waves x 16
#define OTS_RAW LDW_RAW                             // 16 KiB: g of a piece
#define OTS_RING 4
#define OTS_RING_BASE (2 * OTS_XPIECE)              // two image slots, then the ring
#define OTS_LDS (OTS_RING_BASE + OTS_RING * OTS_RAW)   // 136 KiB
#define OTS_MIN_K 32768
#define OTS_MAX_RANGES 64                           // slabs the workspace of pdn_gemm_f32 holds
#define OTS_S_UNSET (1 << 20)                       // the running exponent before the first non-zero piece
#define OTS_S_TOP 15                                // g 2^S stays below 2^15
#define OTS_S_AIM 12                                // a new S puts the piece's maximum into [2^12, 2^13)

// ---- the extra workspace region: [images: K / 32 pieces | 288 exponents] ----------------------------------------------
LDW_HD int64_t ots_extra_bytes(int64_t K) { return (K / LDW_KP) * (int64_t)OTS_XPIECE + LDW_N * 4; }
// (the column-maximum pass parks its partial maxima in the image region, which the plane pass then overwrites: 1152 bytes
// per part, 36 KiB per piece)
LDW_HD int ots_partials(int64_t K) { return ldw_min_i(LDW_MAX_PARTIAL, (int)(K / LDW_KP)); }

// ---- X image: units and fragments are ldw_x_unit / ldw_x_frag ------------------------------------------------------------
// DMA instruction e (0..4) of wave w copies KiB I of the image (waves 4..7 repeat KiB 35 at e = 4: every wave counts alike)
LDW_HD int ots_x_dma_kib(int e, int wave) { return ldw_min_i(e * 8 + wave, OTS_XDMA - 1); }
LDW_HD int64_t ots_x_dma_src(int64_t piece, int I, int lane) { return piece * OTS_XPIECE + I * 1024 + lane * 16; }
LDW_HD int ots_x_dma_lds(int slot, int I, int lane) { return slot * OTS_XPIECE + I * 1024 + lane * 16; }
LDW_HD int ots_x_frag(int slot, int j, int r, int q, int plane) { return slot * OTS_XPIECE + plane * LDW_PLANE + ldw_x_frag(j, r, q); }

// ---- g -------------------------------------------------------------------------------------------------------------------
// DMA instruction i (0, 1) of wave w is KiB I = w + 8 i of the piece: rows 2 I and 2 I + 1, lane l position l & 31, which
// receives chunk (l & 31) ^ swizzle(row) of the row's 32 chunks of 16 bytes
LDW_HD int ots_g_dma_kib(int i, int wave) { return wave + 8 * i; }
LDW_HD int ots_g_dma_row(int I, int lane) { return 2 * I + (lane >> 5); }
LDW_HD int ots_g_dma_chunk(int I, int lane) { return (lane & 31) ^ ldw_raw_swz(ots_g_dma_row(I, lane)); }
LDW_HD int ots_g_dma_lds(int ring, int I, int lane) { return OTS_RING_BASE + ring * OTS_RAW + I * 1024 + lane * 16; }
// first column of the 16 bytes fetched for chunk c of column block bx (past n_all: the row's last chunk, fetched again)
LDW_HD int ots_g_col(int bx, int c, int n_all) { return ldw_min_i(bx * OTS_COLS + 4 * c, n_all - 4); }
// float offset in g of row t of `piece` of a K range of np pieces that begins at token k_begin (past the range: its last
// piece again), first column `col`
LDW_HD int64_t ots_g_src(int k_begin, int piece, int np, int t, int64_t ldg, int col) {
  return ((int64_t)k_begin + (int64_t)ldw_min_i(piece, np - 1) * LDW_KP + t) * ldg + col;
}
// lane (r, q) of wave w reads g of token 8 q + k, column 16 w + r of the block
LDW_HD int ots_g_read(int ring, int wave, int r, int q, int k) {
  const int t = 8 * q + k;
  return OTS_RING_BASE + ring * OTS_RAW + t * 512 + (((4 * wave + (r >> 2)) ^ ldw_raw_swz(t)) << 4) + 4 * (r & 3);
}

// ---- the running exponent of g ---------------------------------------------------------------------------------------------
// `mbits`: the largest |g| of a piece's FINITE values as fp32 bits (0: none, or all zero).  A value with biased exponent E
// lies in [2^(E - 127), 2^(E - 126)) (E = 0: below 2^-126), so g 2^S reaches 2^15 exactly when E - 127 + S >= 15; the new S
// = 139 - E then puts it into [2^12, 2^13).  S only ever falls.
LDW_HD int ots_next_scale(unsigned mbits, int S) {
  if (mbits == 0u) return S;
  const int E = (int)(mbits >> 23);
  return (E - 127 + S >= OTS_S_TOP) ? (OTS_S_AIM + 127 - E) : S;
}

// ---- K ranges and the output -----------------------------------------------------------------------------------------------
// The number of K ranges for n_all columns, given the fp32 kernel's plan and the pieces of K: no fewer than the plan (the
// error is set by the length of the fp32 running sums), no more than the 64 slabs of the workspace (which also bounds the
// plan's own count where that is larger), and within that the most that still fit the whole rounds of 256 workgroups the
// plan's count needs with ceil(n_all / 128) column blocks: 864 columns 7 x 64 = 448 (two rounds, 64 pieces each at 131072
// tokens), 1536 columns 12 x 42 = 504 (two rounds of 98 pieces; 64 ranges would be three rounds of 64 with half as many
// fills and drains again and 1.5 x the slab pass).
LDW_HD int ots_ranges(int n_all, int plan, int pieces) {
  const int cb = (n_all + OTS_COLS - 1) / OTS_COLS;
  const int lo = ldw_min_i(plan, OTS_MAX_RANGES);
  const int rounds = (cb * lo + 255) / 256;
  int r = ldw_min_i(OTS_MAX_RANGES, rounds * 256 / cb);
  if (r < lo) r = lo;
  if (r > pieces) r = pieces;
  return r < 1 ? 1 : r;
}
LDW_HD int ots_k_per_split(int pieces, int ranges) { return ((pieces + ranges - 1) / ranges) * LDW_KP; }
// accumulator register i of tile j in lane (r, q): row ldw_out_row(j, q, i), column `col` of the packed matrix
LDW_HD int64_t ots_out_elem(int by, int64_t slab, int64_t blk_stride, int nb_cols, int d, int col) {
  const int b = col / nb_cols;
  return (int64_t)b * blk_stride + (int64_t)by * slab + (int64_t)d * nb_cols + (col - b * nb_cols);
}
