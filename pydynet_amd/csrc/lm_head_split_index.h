// Index arithmetic of the split-fp16 lm_head forward (csrc/lm_head_split.hip) on `v_mfma_f32_16x16x32_f16`, shared by
// the kernels and the host checker (tests/lm_head_split_m16_check.cpp) that walks every workgroup, wave, lane and tile:
// which global bytes a DMA, a load or a store touches, where they land in LDS, and the swizzle.  Nothing here depends on
// HIP.
//
// A lane of a 16x16x32 operand is (r, q) = (lane & 15, lane >> 4): it holds k = 32 s + 8 q .. + 7 of row r in k-step s
// (a UNIT: 8 halves = 16 bytes; a row / column of 288 has 36 units, unit u = 4 s + q).  In the accumulators lane (r, q)
// holds row r of the B operand (a row of x) and rows 4 q .. 4 q + 3 of the A operand (columns of W).
//   x image of a block of 32 rows (LS_XBLK bytes, written by the x pass, loaded once into a wave's registers):
//     [plane h | plane l], a plane is [k-step s = 9][row half rb = 2][lane = 64][16 bytes]: lane (r, q) of fragment (s, rb)
//     holds unit 4 s + q of row 16 rb + r of the block.
//   W image of a tile of 32 columns (LS_TILE bytes, written by the W pass, copied to LDS as it is):
//     [plane h: 32 x 36 units | plane l | 32 negated exponents | 32 bias values]
//     unit u of column n at n * 36 + (u ^ ((n >> 2) & 3)).  A fragment read (column half c, k-step s) by the sixteen lanes
//     of one q takes unit 4 s + q of columns 16 c + r: with a row stride of 36 units the sixteen addresses fall on
//     sixteen different 16-byte slots of the 256 bytes the banks span.
//   LDS: three slots LS_SLOT apart (37 KiB: a DMA instruction copies 1 KiB, the 37th only its first 256 bytes), then one
//     LS_STG area per wave through which a finished tile leaves row-wise (32 rows of 128 bytes, 16 bytes of padding each).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LSI_HD __host__ __device__ __forceinline__ constexpr
#else
#define LSI_HD inline constexpr
#endif

#define LS_K 288
#define LS_KS 9                           // k-steps of 32
#define LS_UNITS 36                       // 16-byte units of a row of x / a column of W
#define LS_PH 18                          // phases of a tile: (k-step s, column half c), p = 2 s + c
#define LS_PLANE (32 * LS_K * 2)          // bytes of one fp16 plane of a 32-column tile
#define LS_TAIL (2 * LS_PLANE)            // the columns' negated exponents (32 int) and bias (32 float) follow the planes
#define LS_TILE (LS_TAIL + 256)           // bytes of a tile image
#define LS_DMA 37                         // DMA instructions per tile image
#define LS_SLOT (LS_DMA * 1024)           // an LDS slot
#define LS_XBLK (2 * LS_UNITS * 512)      // bytes of the two planes of 32 rows of x
#define LS_STG (32 * 144)                 // a wave's leaving tile on its way out
#define LS_LDS (3 * LS_SLOT + 8 * LS_STG)
#define LS_MIN_ROWS 16384

static_assert(LS_TILE == 37120 && LS_XBLK == 36864 && LS_LDS == 150528 && LS_LDS <= 160 * 1024, "image sizes, LDS allocation");
static_assert(LS_TILE > (LS_DMA - 1) * 1024 && LS_TILE - (LS_DMA - 1) * 1024 == 16 * 16, "the last DMA instruction: sixteen lanes");

// ---- the launch: tiles per workgroup and vocabulary ranges (few rows: the vocabulary is cut into ranges over the grid) --
LSI_HD int64_t ls_mpad(int64_t M) { return (M + 255) / 256 * 256; }
LSI_HD int ls_plan_parts(int64_t M, int V) {
  const int nt = V / 32;
  const int64_t row_blocks = (M + 255) / 256;
  int ns = 1;
  while (row_blocks * ns < 256 && ns < nt) ++ns;
  return ns;
}
LSI_HD int ls_plan_tpw(int64_t M, int V) { return (V / 32 + ls_plan_parts(M, V) - 1) / ls_plan_parts(M, V); }
LSI_HD int ls_plan_ranges(int64_t M, int V) { return (V / 32 + ls_plan_tpw(M, V) - 1) / ls_plan_tpw(M, V); }
// workspace: [W images: V / 32 tiles | x images: Mpad / 32 blocks | Mpad negated exponents]
LSI_HD int64_t ls_workspace_bytes(int64_t M, int V) {
  return (int64_t)(V / 32) * LS_TILE + ls_mpad(M) / 32 * LS_XBLK + ls_mpad(M) * 4;
}

// ---- x image ----------------------------------------------------------------------------------------------------------
// unit u of row rr (0..31) of a block, plane h (plane l: LS_XBLK / 2 further on)
LSI_HD int ls_x_unit(int rr, int u) { return ((2 * (u >> 2) + (rr >> 4)) * 64 + (u & 3) * 16 + (rr & 15)) * 16; }
// fragment (k-step s, row half rb) of a lane
LSI_HD int ls_x_frag(int s, int rb, int lane) { return ((2 * s + rb) * 64 + lane) * 16; }

// ---- W image ----------------------------------------------------------------------------------------------------------
LSI_HD int ls_w_unit(int n, int u) { return (n * LS_UNITS + (u ^ ((n >> 2) & 3))) * 16; }      // byte offset in a plane
// fragment of phase p = 2 s + c for lane (r, q): column 16 c + r, unit 4 s + q = a lane part + a phase part
LSI_HD int ls_w_frag_lane(int lane) { return ((lane & 15) * LS_UNITS + ((lane >> 4) ^ (((lane & 15) >> 2) & 3))) * 16; }
LSI_HD int ls_w_frag_phase(int p) { return (p & 1) * (16 * LS_UNITS * 16) + (p >> 1) * 64; }
// negated exponents of columns 16 c + 4 q .. + 3 (the bias: 128 bytes further on)
LSI_HD int ls_tail_ne(int c, int q) { return LS_TAIL + 64 * c + 16 * q; }

// ---- staging: DMA instruction I (0..36) copies bytes 1024 I + 16 lane of the image to the same offset of the slot; wave
// w issues I = w, w + 8, w + 16, w + 24 and, w < 5, 32 + w ------------------------------------------------------------
LSI_HD int ls_dma_count(int wave) { return wave < LS_DMA - 32 ? 5 : 4; }
LSI_HD int ls_dma_instr(int wave, int e) { return 8 * e + wave; }
LSI_HD int ls_dma_lanes(int I) { return I == LS_DMA - 1 ? (LS_TILE - (LS_DMA - 1) * 1024) / 16 : 64; }
LSI_HD int ls_dma_offset(int I, int lane) { return I * 1024 + lane * 16; }

// ---- the way out ------------------------------------------------------------------------------------------------------
// accumulator group g = 2 c + rb of lane (r, q): row 16 rb + r of the wave's 32, columns 16 c + 4 q .. + 3 of the tile
LSI_HD int ls_acc_row(int g, int lane) { return 16 * (g & 1) + (lane & 15); }
LSI_HD int ls_acc_col(int g, int lane) { return 16 * (g >> 1) + 4 * (lane >> 4); }
LSI_HD int ls_stg_write(int g, int lane) { return ls_acc_row(g, lane) * 144 + ls_acc_col(g, lane) * 4; }
// store j (0..3): rows 8 j + (lane >> 3), eight lanes per 128-byte line
LSI_HD int ls_store_row(int j, int lane) { return 8 * j + (lane >> 3); }
LSI_HD int ls_store_col(int lane) { return 4 * (lane & 7); }
LSI_HD int ls_stg_read(int j, int lane) { return ls_store_row(j, lane) * 144 + ls_store_col(lane) * 4; }
