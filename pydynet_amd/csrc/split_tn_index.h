// Index arithmetic of the split-fp16 TN pipeline (csrc/split_tn.h) and of its two users, the lm_head weight gradient
// (csrc/lm_head_dw_split.hip, LDW_ / ldw_) and the packed layer weight gradients (csrc/outres_tn_split.hip, OTS_ / ots_),
// shared by the kernels and the host checkers (tests/lm_head_dw_split_check.cpp, tests/outres_tn_split_check.cpp,
// tests/down_dw_split_check.cpp: the transposed one-block form and the plane pass) that walk
// every workgroup, wave, lane and piece: which global bytes a DMA or a store touches, where they land in LDS, and the
// swizzles.  Nothing here depends on HIP.
//
// A PIECE is 32 consecutive tokens, one k-step of `v_mfma_f32_16x16x32_f16` (the contraction index is the token).
//   X image of a piece (`xkib` KiB, written once per call by the plane pass, copied to LDS as it is):
//     [plane h: 288 x 4 units | plane l: 288 x 4 units | tail]      a unit = 8 halves = 16 bytes
//     unit q of column d (tokens 8 q .. 8 q + 7 of the piece: what lane quarter q multiplies) at stn_x_unit(d, q);
//     xkib = 36 (OTS_XKIB): the two planes; xkib = 37 (LDW_XKIB): and a tail of 32 floats -lse[t] log2 e, then 32 ints
//     target[t], of the tokens of the NEXT piece (they are needed one piece ahead of the planes: the cross-entropy
//     gradient of piece s + 1 is formed while piece s is multiplied).
//   the raw matrix (the logits, or g) of a piece for a workgroup's 128 columns: 32 rows x 512 bytes in LDS, in a ring of
//     four behind the two image slots; rows `ld` floats apart in memory (ld >= the column count: g may be padded), columns
//     past the last clamped to the row's last 16 bytes.  Row t as 32 chunks of 16 bytes; POSITION p of row t holds chunk
//     p ^ 4 (t >> 3) of the row (the DMA's source side is permuted, its LDS side is linear): lane (r, q) of wave w reads
//     column 16 w + r of tokens 8 q + k, and the four q then sit in four different groups of four chunks: every bank once.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define STN_HD __host__ __device__ __forceinline__ constexpr
#else
#define STN_HD inline constexpr
#endif

#define STN_N 288                                   // rows of dW: 18 tiles of 16
#define STN_NT 18
#define STN_KP 32                                   // tokens per piece
#define STN_PLANE (STN_N * STN_KP * 2)              // bytes of one fp16 plane of a piece
#define STN_COLS 128                                // columns per workgroup: 8 waves x 16
#define STN_RAW (STN_KP * STN_COLS * 4)             // 16 KiB: the raw matrix of a piece
#define STN_RAWDMA 16                               // DMA instructions per piece of the raw matrix
#define STN_RING 4
#define STN_MAX_PARTIAL 2048                        // row ranges of the column-maximum pass

#define LDW_XKIB 37                                 // DMA instructions (1 KiB each) per image: two planes and the tail
#define LDW_TAIL (2 * STN_PLANE)                    // offset of the tail in a piece's image
#define LDW_MIN_ROWS 32768
#define LDW_MIN_V 128

#define OTS_XKIB 36                                 // two planes
#define OTS_MIN_K 32768
#define OTS_MAX_RANGES 64                           // slabs the workspace of pdn_gemm_f32 holds
#define OTS_S_UNSET (1 << 20)                       // the running exponent before the first non-zero piece
#define OTS_S_TOP 15                                // g 2^S stays below 2^15
#define OTS_S_AIM 12                                // a new S puts the piece's maximum into [2^12, 2^13)

STN_HD int stn_min_i(int a, int b) { return a < b ? a : b; }

// ---- LDS: two image slots, then the ring; the extra workspace region: [images: rows / 32 pieces | 288 exponents] ---------
STN_HD int stn_xpiece(int xkib) { return xkib * 1024; }
STN_HD int stn_ring_base(int xkib) { return 2 * stn_xpiece(xkib); }
STN_HD int stn_lds(int xkib) { return stn_ring_base(xkib) + STN_RING * STN_RAW; }
STN_HD int64_t stn_extra_bytes(int64_t rows, int xkib) { return (rows / STN_KP) * (int64_t)stn_xpiece(xkib) + STN_N * 4; }
// (the column-maximum pass parks its partial maxima in the image region, which the plane pass then overwrites: 1152 bytes
// per part, at least 36 KiB per piece)
STN_HD int stn_partials(int64_t rows) { return stn_min_i(STN_MAX_PARTIAL, (int)(rows / STN_KP)); }
// the closed forms that include/pdn_hip.h and the tests quote
static_assert(stn_xpiece(LDW_XKIB) == 37888 && stn_xpiece(OTS_XKIB) == 36864 && STN_N * 4 == 1152, "bytes per piece, exponents");
static_assert(stn_xpiece(OTS_XKIB) == 2 * STN_PLANE && LDW_TAIL + 1024 == stn_xpiece(LDW_XKIB), "an image is two planes, and a tail");
static_assert(stn_lds(LDW_XKIB) == 141312 && stn_lds(OTS_XKIB) == 139264, "LDS allocations");

// ---- X image ---------------------------------------------------------------------------------------------------------
STN_HD int stn_x_unit(int d, int q) { return (d * 4 + (q ^ ((d >> 2) & 3))) * 16; }            // byte offset in a plane
// fragment of tile j for lane (r, q): row d = 16 j + r of the image, unit q
STN_HD int stn_x_frag(int j, int r, int q) { return j * 1024 + (r * 4 + (q ^ ((r >> 2) & 3))) * 16; }
// DMA instruction e (0..4) of wave w copies KiB I of the image (the last waves repeat its last KiB: every wave counts alike)
STN_HD int stn_x_dma_kib(int e, int wave, int xkib) { return stn_min_i(e * 8 + wave, xkib - 1); }
STN_HD int64_t stn_x_dma_src(int64_t piece, int I, int lane, int xkib) { return piece * stn_xpiece(xkib) + I * 1024 + lane * 16; }   // byte in the image region
STN_HD int stn_x_dma_lds(int slot, int I, int lane, int xkib) { return slot * stn_xpiece(xkib) + I * 1024 + lane * 16; }
// The plane pass (csrc/split_tn_planes.hip), 256 threads per piece.  Load item i (nine per thread) is the 16 bytes of token
// row i / 72, float4 chunk i % 72 of the piece, staged raw in LDS: token t, column d at float stn_pass_lds(t, d), its chunk
// moved on by four per quarter of the piece (modulo the row's 72), so that the sixteen columns x four quarters a wave reads
// back sit in 64 different banks (a row is 4.5 x 64 banks: rows of one parity begin at the same bank).  Store item u (4.5
// per thread) is unit u of either plane in IMAGE order, bytes 16 u ..: a wave stores 1 KiB of whole lines.
#define STN_PASS_THREADS 256
#define STN_PASS_LOADS (STN_KP * STN_N / 4 / STN_PASS_THREADS)      // 9
STN_HD int stn_pass_row(int i) { return i / (STN_N / 4); }
STN_HD int stn_pass_chunk(int i) { return i % (STN_N / 4); }
STN_HD int stn_pass_lds(int t, int d) {
  const int c = (d >> 2) + 4 * (t >> 3);
  return t * STN_N + 4 * (c >= STN_N / 4 ? c - STN_N / 4 : c) + (d & 3);
}
STN_HD int stn_pass_unit_d(int u) { return u >> 2; }
STN_HD int stn_pass_unit_q(int u) { return (u & 3) ^ ((u >> 4) & 3); }      // stn_x_unit(d, q) == 16 u
static_assert(STN_PASS_LOADS * STN_PASS_THREADS * 4 == STN_KP * STN_N, "nine whole load items per thread");

STN_HD int ldw_tail_nl(int slot, int t) { return slot * stn_xpiece(LDW_XKIB) + LDW_TAIL + 4 * t; }
STN_HD int ldw_tail_tg(int slot, int t) { return slot * stn_xpiece(LDW_XKIB) + LDW_TAIL + 128 + 4 * t; }

// ---- the raw matrix ----------------------------------------------------------------------------------------------------
// DMA instruction i (0, 1) of wave w is KiB I = w + 8 i of the piece: rows 2 I and 2 I + 1, lane l position l & 31, which
// receives chunk (l & 31) ^ swizzle(row) of the row's 32 chunks of 16 bytes
STN_HD int stn_raw_dma_kib(int i, int wave) { return wave + 8 * i; }
STN_HD int stn_raw_dma_row(int I, int lane) { return 2 * I + (lane >> 5); }
STN_HD int stn_raw_swz(int t) { return 4 * (t >> 3); }
STN_HD int stn_raw_dma_chunk(int I, int lane) { return (lane & 31) ^ stn_raw_swz(stn_raw_dma_row(I, lane)); }
STN_HD int stn_raw_dma_lds(int ring, int I, int lane, int xkib) { return stn_ring_base(xkib) + ring * STN_RAW + I * 1024 + lane * 16; }
// first column of the 16 bytes fetched for chunk c of column block bx (past ncols: the row's last chunk, fetched again)
STN_HD int stn_raw_col(int bx, int c, int ncols) { return stn_min_i(bx * STN_COLS + 4 * c, ncols - 4); }
// token row t of `piece` of a K range of np pieces that begins at token k_begin (past the range: its last piece again), and
// its float offset at first column `col`
STN_HD int64_t stn_raw_row(int k_begin, int piece, int np, int t) { return (int64_t)k_begin + (int64_t)stn_min_i(piece, np - 1) * STN_KP + t; }
STN_HD int64_t stn_raw_src(int k_begin, int piece, int np, int t, int64_t ld, int col) { return stn_raw_row(k_begin, piece, np, t) * ld + col; }
// lane (r, q) of wave w reads token 8 q + k, column 16 w + r of the block
STN_HD int stn_raw_read(int ring, int wave, int r, int q, int k, int xkib) {
  const int t = 8 * q + k;
  return stn_ring_base(xkib) + ring * STN_RAW + t * 512 + (((4 * wave + (r >> 2)) ^ stn_raw_swz(t)) << 4) + 4 * (r & 3);
}

// ---- the running exponent of g ---------------------------------------------------------------------------------------------
// `mbits`: the largest |g| of a piece's FINITE values as fp32 bits (0: none, or all zero).  A value with biased exponent E
// lies in [2^(E - 127), 2^(E - 126)) (E = 0: below 2^-126), so g 2^S reaches 2^15 exactly when E - 127 + S >= 15; the new S
// = 139 - E then puts it into [2^12, 2^13).  S only ever falls.
STN_HD int ots_next_scale(unsigned mbits, int S) {
  if (mbits == 0u) return S;
  const int E = (int)(mbits >> 23);
  return (E - 127 + S >= OTS_S_TOP) ? (OTS_S_AIM + 127 - E) : S;
}

// ---- K ranges and the output -----------------------------------------------------------------------------------------------
STN_HD int stn_range_pieces(int K, int k_per_split, int by) {
  const int b = by * k_per_split, e = stn_min_i(K, b + k_per_split);
  return (e - b) / STN_KP;
}
// The number of K ranges of the packed gradients for n_all columns, given the fp32 kernel's plan and the pieces of K: no
// fewer than the plan (the error is set by the length of the fp32 running sums), no more than the 64 slabs of the workspace
// (which also bounds the plan's own count where that is larger), and within that the most that still fit the whole rounds
// of 256 workgroups the plan's count needs with ceil(n_all / 128) column blocks: 864 columns 7 x 64 = 448 (two rounds, 64
// pieces each at 131072 tokens), 1536 columns 12 x 42 = 504 (two rounds of 98 pieces; 64 ranges would be three rounds of 64
// with half as many fills and drains again and 1.5 x the slab pass).
STN_HD int ots_ranges(int n_all, int plan, int pieces) {
  const int cb = (n_all + STN_COLS - 1) / STN_COLS;
  const int lo = stn_min_i(plan, OTS_MAX_RANGES);
  const int rounds = (cb * lo + 255) / 256;
  int r = stn_min_i(OTS_MAX_RANGES, rounds * 256 / cb);
  if (r < lo) r = lo;
  if (r > pieces) r = pieces;
  return r < 1 ? 1 : r;
}
STN_HD int ots_k_per_split(int pieces, int ranges) { return ((pieces + ranges - 1) / ranges) * STN_KP; }
// The one-block TRANSPOSED form (dW_down^T = g2^T h, M = 512 .. 1024 columns of h): ONE round of workgroups, as many ranges
// as 256 workgroups hold with ceil(M / 128) column blocks (768 columns: 6 x 42 = 252, 98 pieces each at 131072 tokens, the
// length of the fp32 running sums the 1536-column packed product already has; 6 x 64 = 384 would be two rounds of 64).
STN_HD int ots_t_ranges(int n_all, int pieces) {
  const int cb = (n_all + STN_COLS - 1) / STN_COLS;
  int r = stn_min_i(OTS_MAX_RANGES, 256 / cb);
  if (r > pieces) r = pieces;
  return r < 1 ? 1 : r;
}
// its store: the lane's registers i = 0 .. 3 of tile j are rows 16 j + 4 q + i of ONE column, sixteen bytes of row `col` of
// the (n_all x 288) slab of K range `by`: element (col, d) at
STN_HD int64_t ots_out_elem_t(int by, int64_t slab, int d, int col) { return (int64_t)by * slab + (int64_t)col * STN_N + d; }
// accumulator register i of tile j in lane (r, q): row 16 j + 4 q + i of dW, column 16 w + r of the block
STN_HD int stn_out_row(int j, int q, int i) { return 16 * j + 4 * q + i; }
// lm_head: slab of K range `by`, rows of V floats
STN_HD int64_t ldw_out_elem(int by, int64_t slab, int d, int V, int col) { return (int64_t)by * slab + (int64_t)d * V + col; }
// packed: block b = column / nb_cols of K range `by` at b * blk_stride + by * slab, rows of nb_cols floats (the batched
// layout of gemm_splitk_reduce_kernel)
STN_HD int64_t ots_out_elem(int by, int64_t slab, int64_t blk_stride, int nb_cols, int d, int col) {
  const int b = col / nb_cols;
  return (int64_t)b * blk_stride + (int64_t)by * slab + (int64_t)d * nb_cols + (col - b * nb_cols);
}
