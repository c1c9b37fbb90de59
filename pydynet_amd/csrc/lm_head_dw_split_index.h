// Index arithmetic of the split-fp16 lm_head weight gradient (csrc/lm_head_dw_split.hip), shared by the kernels and a host
// checker (tests/lm_head_dw_split_check.cpp) that walks every workgroup, wave, lane and piece: which global bytes a DMA
// or a store touches, where they land in LDS, and the swizzles.  Nothing here depends on HIP.
//
// A PIECE is 32 consecutive tokens, one k-step of `v_mfma_f32_16x16x32_f16` (the contraction index is the token).
//   X image of a piece (LDW_XPIECE = 37 KiB, written once per call by the plane pass, copied to LDS as it is):
//     [plane h: 288 x 4 units | plane l: 288 x 4 units | tail]      a unit = 8 halves = 16 bytes
//     unit q of column d (tokens 8 q .. 8 q + 7 of the piece: what lane quarter q multiplies) at ldw_x_unit(d, q);
//     tail: 32 floats -lse[t] log2 e, then 32 ints target[t], of the tokens of the NEXT piece (they are needed one
//     piece ahead of the planes: the cross-entropy gradient of piece s + 1 is formed while piece s is multiplied).
//   logits of a piece for a workgroup's 128 columns: 32 rows x 512 bytes in LDS, row t as 32 chunks of 16 bytes; POSITION
//     p of row t holds chunk p ^ 4 (t >> 3) of the row (the DMA's source side is permuted, its LDS side is linear):
//     lane (r, q) of wave w reads column 16 w + r of tokens 8 q + k, and the four q then sit in four different groups of
//     four chunks: every bank once.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDW_HD __host__ __device__ __forceinline__
#else
#define LDW_HD inline
#endif

#define LDW_N 288                                   // rows of dW: 18 tiles of 16
#define LDW_NT 18
#define LDW_KP 32                                   // tokens per piece
#define LDW_PLANE (LDW_N * LDW_KP * 2)              // bytes of one fp16 plane of a piece
#define LDW_TAIL (2 * LDW_PLANE)                    // offset of the tail in a piece's image
#define LDW_XDMA 37                                 // DMA instructions (1 KiB each) per image
#define LDW_XPIECE (LDW_XDMA * 1024)                // 37 KiB
#define LDW_COLS 128                                // vocabulary columns per workgroup: 8 waves x 16
#define LDW_RAW (LDW_KP * LDW_COLS * 4)             // 16 KiB: the logits of a piece
#define LDW_RAWDMA 16                               // DMA instructions per piece of logits
#define LDW_RING 4
#define LDW_RING_BASE (2 * LDW_XPIECE)              // two image slots, then the ring
#define LDW_LDS (LDW_RING_BASE + LDW_RING * LDW_RAW)   // 138 KiB
#define LDW_MIN_ROWS 32768
#define LDW_MIN_V 128
#define LDW_MAX_PARTIAL 2048                        // row ranges of the column-maximum pass

LDW_HD int ldw_min_i(int a, int b) { return a < b ? a : b; }

// ---- the extra workspace region: [images: rows / 32 pieces | 288 exponents] --------------------------------------------
LDW_HD int64_t ldw_extra_bytes(int64_t rows) { return (rows / LDW_KP) * (int64_t)LDW_XPIECE + LDW_N * 4; }
// (the column-maximum pass parks its partial maxima in the image region, which the plane pass then overwrites)
LDW_HD int ldw_partials(int64_t rows) { return ldw_min_i(LDW_MAX_PARTIAL, (int)(rows / LDW_KP)); }

// ---- X image ---------------------------------------------------------------------------------------------------------
LDW_HD int ldw_x_unit(int d, int q) { return (d * 4 + (q ^ ((d >> 2) & 3))) * 16; }            // byte offset in a plane
// fragment of tile j for lane (r, q): row d = 16 j + r of the image, unit q
LDW_HD int ldw_x_frag(int j, int r, int q) { return j * 1024 + (r * 4 + (q ^ ((r >> 2) & 3))) * 16; }
// DMA instruction e (0..4) of wave w copies KiB I of the image (the last waves repeat KiB 36: every wave counts alike)
LDW_HD int ldw_x_dma_kib(int e, int wave) { return ldw_min_i(e * 8 + wave, LDW_XDMA - 1); }
LDW_HD int64_t ldw_x_dma_src(int64_t piece, int I, int lane) { return piece * LDW_XPIECE + I * 1024 + lane * 16; }   // byte in the image region
LDW_HD int ldw_x_dma_lds(int slot, int I, int lane) { return slot * LDW_XPIECE + I * 1024 + lane * 16; }
LDW_HD int ldw_tail_nl(int slot, int t) { return slot * LDW_XPIECE + LDW_TAIL + 4 * t; }
LDW_HD int ldw_tail_tg(int slot, int t) { return slot * LDW_XPIECE + LDW_TAIL + 128 + 4 * t; }

// ---- logits ----------------------------------------------------------------------------------------------------------
// DMA instruction i (0, 1) of wave w is KiB I = w + 8 i of the piece: rows 2 I and 2 I + 1, lane l position l & 31
LDW_HD int ldw_raw_dma_kib(int i, int wave) { return wave + 8 * i; }
LDW_HD int ldw_raw_dma_row(int I, int lane) { return 2 * I + (lane >> 5); }
LDW_HD int ldw_raw_swz(int t) { return 4 * (t >> 3); }
LDW_HD int ldw_raw_dma_chunk(int I, int lane) { return (lane & 31) ^ ldw_raw_swz(ldw_raw_dma_row(I, lane)); }
LDW_HD int ldw_raw_dma_lds(int ring, int I, int lane) { return LDW_RING_BASE + ring * LDW_RAW + I * 1024 + lane * 16; }
// first column of the 16 bytes fetched for chunk c of column block bx (past V: the row's last chunk, fetched again)
LDW_HD int ldw_raw_col(int bx, int c, int V) { return ldw_min_i(bx * LDW_COLS + 4 * c, V - 4); }
// token row of `piece` of a K range of np pieces that begins at token k_begin (past the range: its last piece again)
LDW_HD int64_t ldw_raw_row(int k_begin, int piece, int np, int t) { return (int64_t)k_begin + (int64_t)ldw_min_i(piece, np - 1) * LDW_KP + t; }
// lane (r, q) of wave w reads the logit of token 8 q + k, column 16 w + r of the block
LDW_HD int ldw_raw_read(int ring, int wave, int r, int q, int k) {
  const int t = 8 * q + k;
  return LDW_RING_BASE + ring * LDW_RAW + t * 512 + (((4 * wave + (r >> 2)) ^ ldw_raw_swz(t)) << 4) + 4 * (r & 3);
}

// ---- K ranges and the output -----------------------------------------------------------------------------------------
LDW_HD int ldw_range_pieces(int K, int k_per_split, int by) {
  const int b = by * k_per_split, e = ldw_min_i(K, b + k_per_split);
  return (e - b) / LDW_KP;
}
// accumulator register i of tile j in lane (r, q): row 16 j + 4 q + i of dW, column 16 w + r of the block
LDW_HD int ldw_out_row(int j, int q, int i) { return 16 * j + 4 * q + i; }
LDW_HD int64_t ldw_out_elem(int by, int64_t slab, int d, int V, int col) { return (int64_t)by * slab + (int64_t)d * V + col; }
