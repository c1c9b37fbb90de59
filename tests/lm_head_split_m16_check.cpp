// Host checker of the split-fp16 lm_head forward's index arithmetic (pydynet_amd/csrc/lm_head_split_index.h, the header
// from which csrc/lm_head_split.hip takes every address it forms).  Built with the host compiler and
// -fsanitize=address,undefined by tests/test_lm_head_split_m16_check_cpu.py and run as a process of its own.  Once for
// the layouts, and for every shape on the command line (`M V`, pairs), it walks every workgroup, wave, lane and tile and
// asserts that
//   * every global byte range the passes and the product kernel form lies inside its buffer;
//   * every LDS offset lies inside the allocation, and inside the region it is meant for;
//   * every 16-byte unit of a W tile image is staged exactly once;
//   * the image the split passes write is what the fragment reads address: lane (r, q) of fragment (k-step s, half) finds
//     k = 32 s + 8 q .. + 7 of row / column 16 half + r;
//   * the sixteen lanes of each quarter of a fragment read fall on sixteen different 16-byte bank slots;
//   * every logit of rows below M and columns below V is stored exactly once and nothing at or beyond M is stored (rows and
//     column chunks each covered once for every shape; every element counted where M V <= 2^30 + 2^27).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pydynet_amd/csrc/lm_head_split_index.h"

#define CHECK(c, ...)                                                                  \
  do {                                                                                 \
    if (!(c)) {                                                                        \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s\n  ", __FILE__, __LINE__, #c);   \
      std::fprintf(stderr, __VA_ARGS__);                                               \
      std::fprintf(stderr, "\n");                                                      \
      std::fflush(stderr);                                                             \
      std::_Exit(1);                                                                   \
    }                                                                                  \
  } while (0)

static void check_layouts() {
  // x image: the 36 units of 32 rows fill a plane exactly once; the fragments address what the pass wrote
  std::vector<int> seen(LS_XBLK / 2 / 16, 0);
  for (int rr = 0; rr < 32; ++rr)
    for (int u = 0; u < LS_UNITS; ++u) {
      const int o = ls_x_unit(rr, u);
      CHECK(o >= 0 && o % 16 == 0 && o + 16 <= LS_XBLK / 2, "x unit (%d, %d) at %d", rr, u, o);
      CHECK(!seen[o / 16]++, "x unit (%d, %d) at %d written twice", rr, u, o);
    }
  for (int s = 0; s < LS_KS; ++s)
    for (int rb = 0; rb < 2; ++rb)
      for (int l = 0; l < 64; ++l)
        CHECK(ls_x_frag(s, rb, l) == ls_x_unit(16 * rb + (l & 15), 4 * s + (l >> 4)), "x fragment (%d, %d) lane %d", s, rb, l);
  // W image: 32 columns x 36 units fill a plane exactly once
  seen.assign(LS_PLANE / 16, 0);
  for (int n = 0; n < 32; ++n)
    for (int u = 0; u < LS_UNITS; ++u) {
      const int o = ls_w_unit(n, u);
      CHECK(o >= 0 && o % 16 == 0 && o + 16 <= LS_PLANE, "W unit (%d, %d) at %d", n, u, o);
      CHECK(!seen[o / 16]++, "W unit (%d, %d) at %d written twice", n, u, o);
    }
  // fragments of the 18 phases: the right unit, inside the plane, each quarter of the wave on sixteen bank slots
  for (int slot = 0; slot < 3; ++slot)
    for (int p = 0; p < LS_PH; ++p)
      for (int q = 0; q < 4; ++q) {
        int slots = 0;
        for (int r = 0; r < 16; ++r) {
          const int l = 16 * q + r, o = ls_w_frag_lane(l) + ls_w_frag_phase(p);
          CHECK(o == ls_w_unit(16 * (p & 1) + r, 4 * (p >> 1) + q), "W fragment phase %d lane %d at %d", p, l, o);
          for (int plane = 0; plane < 2; ++plane) {
            const int a = slot * LS_SLOT + plane * LS_PLANE + o;
            CHECK(a >= slot * LS_SLOT && a + 16 <= slot * LS_SLOT + LS_TAIL && a + 16 <= LS_LDS, "fragment read at %d", a);
          }
          slots |= 1 << (((slot * LS_SLOT + o) / 16) & 15);
        }
        CHECK(slots == 0xffff, "phase %d quarter %d: bank slots %04x", p, q, slots);
      }
  // the tail reads: exponents and bias of the lane's four columns
  for (int c = 0; c < 2; ++c)
    for (int q = 0; q < 4; ++q) {
      const int a = ls_tail_ne(c, q);
      CHECK(a == LS_TAIL + 4 * (16 * c + 4 * q) && a + 16 <= LS_TAIL + 128 && a + 128 + 16 <= LS_TILE, "tail (%d, %d) at %d", c, q, a);
    }
  // staging: every 16-byte unit of an image copied exactly once, to the same offset of a slot, inside the slot
  seen.assign(LS_TILE / 16, 0);
  int instr = 0;
  for (int w = 0; w < 8; ++w)
    for (int e = 0; e < ls_dma_count(w); ++e) {
      const int I = ls_dma_instr(w, e);
      CHECK(I >= 0 && I < LS_DMA && e < 5, "wave %d instruction %d", w, I);
      ++instr;
      for (int l = 0; l < ls_dma_lanes(I); ++l) {
        const int o = ls_dma_offset(I, l);
        CHECK(o >= 0 && o + 16 <= LS_TILE && o + 16 <= LS_SLOT, "DMA %d lane %d at %d", I, l, o);
        CHECK(!seen[o / 16]++, "unit %d staged twice", o / 16);
      }
    }
  CHECK(instr == LS_DMA, "%d DMA instructions", instr);
  for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "unit %zu staged %d times", i, seen[i]);
  CHECK(3 * LS_SLOT + 8 * LS_STG == LS_LDS, "LDS allocation");
  // the leaving tile: the four groups fill 32 rows x 128 bytes of the wave's area once (each quarter of the wave on sixteen
  // bank slots), and the row-wise reads take each 16 bytes once
  seen.assign(32 * 8, 0);
  std::vector<int> taken(32 * 8, 0);
  for (int g = 0; g < 4; ++g)
    for (int q = 0; q < 4; ++q) {
      int slots = 0;
      for (int r = 0; r < 16; ++r) {
        const int l = 16 * q + r, o = ls_stg_write(g, l), row = ls_acc_row(g, l), col = ls_acc_col(g, l);
        CHECK(row >= 0 && row < 32 && col >= 0 && col % 4 == 0 && col + 4 <= 32, "group %d lane %d: (%d, %d)", g, l, row, col);
        CHECK(o == row * 144 + col * 4 && o + 16 <= LS_STG, "group %d lane %d at %d", g, l, o);
        CHECK(!seen[row * 8 + col / 4]++, "(%d, %d) written twice", row, col);
        slots |= 1 << ((o / 16) & 15);
      }
      CHECK(slots == 0xffff, "group %d quarter %d: bank slots %04x", g, q, slots);
    }
  for (int j = 0; j < 4; ++j)
    for (int l = 0; l < 64; ++l) {
      const int o = ls_stg_read(j, l), row = ls_store_row(j, l), col = ls_store_col(l);
      CHECK(row >= 0 && row < 32 && col % 4 == 0 && col + 4 <= 32 && o == row * 144 + col * 4 && o + 16 <= LS_STG, "store %d lane %d", j, l);
      CHECK(seen[row * 8 + col / 4] == 1 && !taken[row * 8 + col / 4]++, "(%d, %d) read twice or never written", row, col);
    }
  for (size_t i = 0; i < taken.size(); ++i) CHECK(taken[i] == 1, "chunk %zu of the leaving tile read %d times", i, taken[i]);
}

static void check_shape(int64_t M, int V, int64_t ldl) {
  CHECK(M >= LS_MIN_ROWS && V >= 32 && V % 32 == 0 && ldl >= V && ldl % 4 == 0 && ldl < (1 << 24), "unsupported shape %lld x %d", (long long)M, V);
  const int64_t mp = ls_mpad(M), ws = ls_workspace_bytes(M, V);
  const int nt = V / 32, tpw = ls_plan_tpw(M, V), parts = ls_plan_ranges(M, V);
  CHECK(mp % 256 == 0 && mp >= M && mp - M < 256, "Mpad %lld", (long long)mp);
  CHECK(tpw >= 1 && parts >= 1 && (int64_t)(parts - 1) * tpw < nt && (int64_t)parts * tpw >= nt, "plan: %d ranges of %d tiles", parts, tpw);
  const int64_t wimg = 0, ximg = (int64_t)nt * LS_TILE, nex = ximg + mp / 32 * LS_XBLK;
  CHECK(nex + mp * 4 == ws && ximg % 16 == 0 && nex % 16 == 0, "workspace regions");
  const int64_t c_bytes = ((M - 1) * ldl + V) * 4;          // the logits: rows ldl floats apart, the last one V long

  // the W pass (one workgroup per tile) and the x pass (one wave per row of Mpad)
  for (int t = 0; t < nt; ++t) {
    const int64_t b = wimg + (int64_t)t * LS_TILE;
    CHECK(b >= 0 && b + LS_TILE <= ximg, "W image %d", t);
    CHECK(32 * t + 31 < V, "columns of tile %d", t);
  }
  for (int64_t row = 0; row < mp; ++row) {
    const int64_t lo = ximg + (row >> 5) * LS_XBLK + ls_x_unit((int)(row & 31), 0);
    const int64_t hi = ximg + (row >> 5) * LS_XBLK + LS_XBLK / 2 + ls_x_unit((int)(row & 31), LS_UNITS - 1) + 16;
    CHECK(lo >= ximg && hi <= nex, "x image of row %lld", (long long)row);
    CHECK(nex + row * 4 + 4 <= ws, "exponent of row %lld", (long long)row);
  }

  // the product kernel
  const int64_t nbx = mp / 256;
  std::vector<uint8_t> row_stored((size_t)mp, 0), chunk_stored((size_t)(V / 4), 0), max_stored((size_t)parts * M, 0);
  const bool every = (double)M * V <= 1024.0 * 1024 * 1024 + 128.0 * 1024 * 1024;
  std::vector<uint8_t> stored(every ? (size_t)(M * (int64_t)(V / 4)) : 0, 0);
  int64_t tiles = 0;
  for (int by = 0; by < parts; ++by) {
    const int T0 = by * tpw, T1 = nt < T0 + tpw ? nt : T0 + tpw;
    CHECK(T0 < T1, "range %d is empty", by);
    tiles += T1 - T0;
    for (int t = T0; t < T1; ++t) {
      for (int I = 0; I < LS_DMA; ++I) {
        const int64_t a = wimg + (int64_t)t * LS_TILE + ls_dma_offset(I, ls_dma_lanes(I) - 1) + 16;
        CHECK(a <= ximg, "DMA source of tile %d", t);
      }
      for (int l = 0; l < 8; ++l) {
        const int col = 32 * t + ls_store_col(l);
        CHECK(col + 4 <= V, "column %d", col);
        CHECK(!chunk_stored[col / 4]++, "columns %d .. stored twice", col);
      }
    }
  }
  CHECK(tiles == nt, "the ranges hold %lld tiles of %d", (long long)tiles, nt);
  for (int64_t bx = 0; bx < nbx; ++bx)
    for (int w = 0; w < 8; ++w) {
      const int64_t blk = bx * 8 + w, m0 = blk * 32;
      for (int s = 0; s < LS_KS; ++s)
        for (int rb = 0; rb < 2; ++rb) {
          const int64_t a = ximg + blk * LS_XBLK + LS_XBLK / 2 + ls_x_frag(s, rb, 63) + 16;
          CHECK(a <= nex, "x fragments of block %lld", (long long)blk);
        }
      for (int l = 0; l < 64; ++l) {
        for (int rb = 0; rb < 2; ++rb) {
          const int64_t row = m0 + 16 * rb + (l & 15);
          CHECK(nex + row * 4 + 4 <= ws, "exponent read of row %lld", (long long)row);
          if ((l >> 4) == 0 && row < M)
            for (int by = 0; by < parts; ++by) {
              const int64_t o = (int64_t)by * M + row;
              CHECK(o < (int64_t)parts * M && !max_stored[o]++, "row maximum %lld", (long long)o);
            }
        }
        for (int j = 0; j < 4; ++j) {
          const int64_t row = m0 + ls_store_row(j, l);
          // the kernel's 32-bit byte offset beside the wave's base
          const uint64_t ob = 4ull * (uint64_t)ls_store_row(0, l) * (uint64_t)ldl + 4ull * ls_store_col(l) + (uint64_t)j * 32ull * (uint64_t)ldl;
          CHECK(ob < (1ull << 32) && ob == 4ull * ((uint64_t)ls_store_row(j, l) * (uint64_t)ldl + ls_store_col(l)), "store offset");
          if (row >= M) continue;                               // GUARD: never stored
          if ((l & 7) == 0) CHECK(!row_stored[row]++, "row %lld stored twice", (long long)row);
          const int64_t last = ((row * ldl) + 32 * (int64_t)(nt - 1) + ls_store_col(l)) * 4 + 16;
          CHECK(last <= c_bytes, "store of row %lld", (long long)row);
          if (every)
            for (int t = 0; t < nt; ++t) {
              const int64_t o = row * (V / 4) + (32 * t + ls_store_col(l)) / 4;
              CHECK(!stored[o]++, "chunk %lld stored twice", (long long)o);
            }
        }
      }
    }
  for (int64_t r = 0; r < mp; ++r) CHECK(row_stored[r] == (r < M ? 1 : 0), "row %lld stored %d times", (long long)r, row_stored[r]);
  for (size_t c = 0; c < chunk_stored.size(); ++c) CHECK(chunk_stored[c] == 1, "chunk column %zu stored %d times", c, chunk_stored[c]);
  for (size_t o = 0; o < max_stored.size(); ++o) CHECK(max_stored[o] == 1, "row maximum %zu stored %d times", o, max_stored[o]);
  for (size_t o = 0; o < stored.size(); ++o) CHECK(stored[o] == 1, "chunk %zu stored %d times", o, stored[o]);
  std::printf("M %lld V %d ldl %lld: %d ranges of %d tiles, %lld workgroups; every logit stored once%s, none beyond M; %d row maxima per row\n",
              (long long)M, V, (long long)ldl, parts, tpw, (long long)(nbx * parts), every ? " (every element counted)" : "", parts);
}

int main(int argc, char** argv) {
  check_layouts();
  std::printf("layouts: x and W images, fragments, tail, staging and the leaving tile agree; fragment reads free of bank conflicts\n");
  CHECK(argc >= 3 && argc % 2 == 1, "usage: %s M V [M V ..]", argv[0]);
  for (int a = 1; a + 1 < argc; a += 2) {
    const int64_t M = std::atoll(argv[a]);
    const int V = std::atoi(argv[a + 1]);
    check_shape(M, V, V);
    check_shape(M, V, V + 32);
  }
  return 0;
}
