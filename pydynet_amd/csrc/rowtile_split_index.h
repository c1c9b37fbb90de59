// Index arithmetic of the split-fp16 q | k | v and gate | up projections (csrc/rowtile_split.hip), shared by the kernels and a
// host checker (tests/rowtile_split_check.cpp) that walks every workgroup, wave, lane, tile and drain step: which global
// elements a load or a store touches, where a value lies in LDS, and the swizzle.  Nothing here depends on HIP.
//
// A TILE is 32 columns of the product over the whole contraction (288).  Its image (RTS_TILE = 36.25 KiB, built once per
// call by the W pass, copied to LDS as it is) has the layout of csrc/lm_head_split.hip:
//   [plane h: 32 rows x 36 units | plane l: the same | 32 negated exponents | 32 zeros (bias)]    a unit = 8 halves of k
//   unit u of tile column n at rts_img_unit(n, u).
// Which columns of the weights a tile holds:
//   q | k | v (kind 3): columns 32 t .. 32 t + 31 of [Wq | Wk | Wv], blocks `bstride` floats apart;
//   gate | up (kind 1): gate columns 16 t .. 16 t + 15 followed by the up columns 16 t .. 16 t + 15.  In the transposed
//     accumulators a lane owns a row and its registers 4 g .. 4 g + 3 are tile columns 8 g + 4 lh .. + 3, so gate[c] is
//     register i and up[c] register i + 8 of the SAME lane: SwiGLU needs no other lane and no third accumulator set, and a
//     cut of the tiles over grid.y cannot separate a gate column from its up column.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTS_HD __host__ __device__ __forceinline__
#else
#define RTS_HD inline
#endif

#define RTS_K 288
#define RTS_KS 18                           // k-steps of 16
#define RTS_PLANE (32 * RTS_K * 2)          // bytes of one fp16 plane of a tile
#define RTS_TAIL (2 * RTS_PLANE)            // the columns' negated exponents (32 int), then 32 zeros
#define RTS_TILE (RTS_TAIL + 256)           // 37120 bytes
#define RTS_UNITS (RTS_TILE / 16)           // 2320 units of 16 bytes
#define RTS_STG (32 * 144)                  // a wave's leaving tile: 32 rows of 32 floats, 16 bytes of padding each
#define RTS_LDS (3 * RTS_TILE + 8 * RTS_STG)   // 144.75 KiB: a ring of three images, eight staging areas
#define RTS_MIN_ROWS 16384

RTS_HD int rts_min_i(int a, int b) { return a < b ? a : b; }

// ---- plan: workgroups of 256 rows; with few rows the tiles are cut into ranges over grid.y ---------------------------
RTS_HD void rts_plan(int64_t M, int ntiles, int* tpw, int* parts) {
  const int64_t row_blocks = (M + 255) / 256;
  int ns = 1;
  while (row_blocks * ns < 256 && ns < ntiles) ++ns;
  const int per = (ntiles + ns - 1) / ns;
  *tpw = per; *parts = (ntiles + per - 1) / per;
}

// ---- W ----------------------------------------------------------------------------------------------------------
// float offset (from the lowest weight block) of contraction row k of tile column n; ldb = floats between two rows of a
// block.  kind 3: nper = columns per block, bstride = floats between blocks; kind 1: g_off / u_off = where the gate / up
// matrix begins.
RTS_HD int64_t rts_w_src(int kind, int tile, int n, int k, int nper, int64_t ldb, int64_t bstride, unsigned g_off, unsigned u_off) {
  if (kind == 1) return (int64_t)(n < 16 ? g_off : u_off) + (int64_t)k * ldb + 16 * tile + (n & 15);
  const int c = 32 * tile + n, b = c / nper;
  return (int64_t)b * bstride + (int64_t)k * ldb + (c - b * nper);
}
// dh + SwiGLU backward (kind 2): the tile's columns are ROWS 32 t .. 32 t + 31 of W_down (F x 288, row-major, ldb floats
// between rows); the W pass reads element i = 0 .. 32 * 288 - 1 of a tile along k: (n, k) = (rts_w_t_n(i), rts_w_t_k(i))
RTS_HD int64_t rts_w_src_t(int tile, int n, int k, int64_t ldb) { return (int64_t)(32 * tile + n) * ldb + k; }
RTS_HD int rts_w_t_n(int i) { return i / RTS_K; }
RTS_HD int rts_w_t_k(int i) { return i % RTS_K; }
// byte offset, inside a plane, of unit u (k = 8 u .. 8 u + 7) of tile column n: with a row stride of 36 units the sixteen
// lanes a ds_read_b128 serves together fall on sixteen different 16-byte slots
RTS_HD int rts_img_unit(int n, int u) { return (n * 36 + (u ^ ((n >> 2) & 3))) * 16; }
// what the product kernel reads for k-step s: lane (li, lh) wants unit 2 s + lh of column li.  The kernel keeps the two
// bases rts_frag_base(li, lh, 0 / 1) and adds the constant rts_frag_step(s).
RTS_HD int rts_frag_base(int li, int lh, int odd) { return rts_img_unit(li, 2 * odd + lh); }
RTS_HD int rts_frag_step(int s) { return ((2 * s) & ~3) * 16; }
// staging of an image, global -> registers -> LDS: unit q * 512 + tid by instruction q (the fifth: 272 threads)
RTS_HD int rts_stage_unit(int q, int tid) { return q * 512 + tid; }
RTS_HD bool rts_stage_on(int q, int tid) { return rts_stage_unit(q, tid) < RTS_UNITS; }

// ---- A: lane (li, lh) of a wave holds k = 16 s + 8 lh .. + 7 of row m0 + li (the B fragment of the f16 32x32x16 MFMA) ---
RTS_HD int rts_a_col(int s, int lh) { return 16 * s + 8 * lh; }
RTS_HD int64_t rts_a_row(int64_t m0, int li, int64_t M) { return m0 + li < M ? m0 + li : M - 1; }

// The kernel no longer loads A through rts_a_col (it still clamps rows with rts_a_row, and its W fragments still meet
// k = rts_a_col(s, lh)): it reads whole 128-byte lines.  Load (c, i) of a lane, c = 0 .. RTS_CHUNKS - 1 (a chunk = 32
// columns = two k-steps), i = 0 .. 3: row rts_pl_row(lane, i) of the wave's 32, columns rts_pl_col(lane, c) .. + 3; the
// eight lanes 8 r .. 8 r + 7 cover one line.  xn leaves from the same places.  The rows' (r, shift) pass from the lanes
// (lane & 7) == 0 to the fragment-owning lanes through rts_pl_stat(row) of the wave's staging area; then chunk c is written
// there at rts_pl_stg_w(lane, i) (row pitch 144 bytes) and k = 32 c + 16 e + 8 lh + 4 half .. + 3 of row li read back from
// rts_pl_stg_r(li, lh, e, half): e = the k-step's parity, the two halves are the fragment's eight values.
#define RTS_CHUNKS 9
RTS_HD int rts_pl_row(int lane, int i) { return (lane >> 3) + 8 * i; }
RTS_HD int rts_pl_col(int lane, int c) { return 32 * c + 4 * (lane & 7); }
RTS_HD int rts_pl_stat(int row) { return row * 16; }
RTS_HD int rts_pl_stg_w(int lane, int i) { return rts_pl_row(lane, i) * 144 + (lane & 7) * 16; }
RTS_HD int rts_pl_stg_r(int li, int lh, int e, int half) { return li * 144 + 64 * e + 32 * lh + 16 * half; }

// ---- the leaving tile: registers -> the wave's staging area -> memory, ROW-wise -----------------------------------------
// group g (registers 4 g .. 4 g + 3 of lane (li, lh)) = tile columns 8 g + 4 lh .. + 3 of row li
RTS_HD int rts_reg_col(int g, int lh) { return 8 * g + 4 * lh; }
RTS_HD int rts_stg_w(int li, int lh, int g) { return li * 144 + 16 * lh + 32 * g; }
// store j (0..3): lane reads row 8 j + (lane >> 3), tile columns 4 (lane & 7) .. + 3
RTS_HD int rts_stg_r(int lane, int j) { return ((lane >> 3) + 8 * j) * 144 + (lane & 7) * 16; }
RTS_HD int rts_st_row(int lane, int j) { return (lane >> 3) + 8 * j; }
RTS_HD int rts_st_col(int lane) { return 4 * (lane & 7); }
// output column of tile column c: q | k | v: 32 t + c; gate | up (packed [gate | up], F columns each): 16 t + c, F + 16 t + c - 16
RTS_HD int rts_out_col(int kind, int tile, int c, int F) { return kind == 1 ? (c < 16 ? 16 * tile + c : F + 16 * tile + c - 16) : 32 * tile + c; }
// dh + SwiGLU backward: tile column c is dh column 32 t + c; store j of a lane (rts_st_row, rts_st_col) reads gate and up
// and writes dgate and dup at the SAME row and these columns of the packed (M x 2F) [gate | up] matrices: eight lanes
// cover one 128-byte line in each of the four streams
RTS_HD int rts_bwd_gate_col(int tile, int c) { return 32 * tile + c; }
RTS_HD int rts_bwd_up_col(int tile, int c, int F) { return F + 32 * tile + c; }
// h = silu(gate) up of a gate | up tile (16 columns): group g (0, 1) of lane (li, lh) = h columns 8 g + 4 lh .. + 3 from
// registers 4 g .. + 3 (gate) and 4 g + 8 .. + 3 (up); it passes through the first 64 bytes of the staging rows AFTER the
// gu stores have read them; store j (0, 1): lane reads row 16 j + (lane >> 2), h columns 4 (lane & 3) .. + 3
RTS_HD int rts_h_w(int li, int lh, int g) { return li * 144 + 16 * lh + 32 * g; }
RTS_HD int rts_h_r(int lane, int j) { return ((lane >> 2) + 16 * j) * 144 + (lane & 3) * 16; }
RTS_HD int rts_h_row(int lane, int j) { return (lane >> 2) + 16 * j; }
RTS_HD int rts_h_col(int tile, int lane) { return 16 * tile + 4 * (lane & 3); }

// ---- RoPE: the (L x hd x 2) table of pdn_rope_table_f32, entry (pos, col) = (cos, col odd ? sin : -sin) -------------------
// group g of lane (li, lh) rotates the pairs (c, c + 1), (c + 2, c + 3), c = 32 t + 8 g + 4 lh (hd a multiple of 4: all
// four inside one head); it needs the entries of the two EVEN columns: float offset of the first, the second 4 floats on
RTS_HD int rts_rope_colh(int tile, int g, int lh, int hd) { return (32 * tile + 8 * g + 4 * lh) % hd; }
// the same without a division, as the kernel forms it: magic = ceil(2^32 / hd) (exact for columns below 65536)
RTS_HD unsigned rts_rope_magic(int hd) { return (unsigned)(((1ull << 32) + (unsigned)hd - 1) / (unsigned)hd); }
RTS_HD unsigned rts_rope_colh_magic(unsigned col, unsigned hd, unsigned magic) {
  return col - hd * (unsigned)(((uint64_t)col * magic) >> 32);
}
RTS_HD int rts_rope_pos(int64_t m0, int li, int L) { return (int)((m0 + li) % L); }
RTS_HD int rts_rope_entry(int pos, int colh, int hd) { return (pos * hd + colh) * 2; }
