// What the two host checkers of the split-fp16 TN pipeline share (tests/lm_head_dw_split_check.cpp,
// tests/outres_tn_split_check.cpp): the fp32 kernel's K plan, the walk over an X image, its DMA and its fragment reads, the
// ring's DMA against its transposed read, and the walk over a K range's fetches.  All of it on
// pydynet_amd/csrc/split_tn_index.h, the header the kernels use; `xkib` is the image size of the kernel under check.
#pragma once
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../pydynet_amd/csrc/split_tn_index.h"

#define CHECK(c, ...)                                                                                   \
  do {                                                                                                  \
    if (!(c)) {                                                                                         \
      std::fprintf(stderr, "CHECK failed at %s:%d: %s\n  ", __FILE__, __LINE__, #c);                    \
      std::fprintf(stderr, __VA_ARGS__);                                                                \
      std::fprintf(stderr, "\n");                                                                       \
      std::fflush(stderr);                                                                              \
      std::_Exit(1);                                                                                    \
    }                                                                                                   \
  } while (0)

// the K ranges of the fp32 kernel (pdn_gemm_outres_tn_plan of csrc/gemm_outres.hip at its default of eight waves)
static int plan(int N, int K, int* kps_out = nullptr) {
  const int col_wgs = (N / 32 + 7) / 8;
  int splits = 256 / (col_wgs > 0 ? col_wgs : 1);
  if (splits < 1) splits = 1;
  if (splits >= 16 && col_wgs > 1) splits &= ~7;
  const int pieces = K / 32;
  if (splits > pieces) splits = pieces > 0 ? pieces : 1;
  const int kps = ((pieces + splits - 1) / splits) * 32;
  if (kps_out) *kps_out = kps;
  return (K + kps - 1) / kps;
}

// ---- shape independent: the image, its DMA, the fragment reads ---------------------------------------------------------
static void check_x_image(int xkib) {
  const int XPIECE = stn_xpiece(xkib);
  CHECK(stn_lds(xkib) <= 160 * 1024, "LDS allocation");
  CHECK(stn_ring_base(xkib) % 1024 == 0 && XPIECE % 1024 == 0 && STN_RAW % 1024 == 0, "DMA granularity");
  // plane pass: thread item i -> (d, q) -> two units; behind the planes the tail, 256 dwords per KiB
  std::vector<int> owner(XPIECE, 0);
  std::vector<int> unit_of(STN_PLANE / 16, -1);
  for (int i = 0; i < STN_N * 4; ++i) {
    const int d = i % STN_N, q = i / STN_N, u = stn_x_unit(d, q);
    CHECK(u >= 0 && u + 16 <= STN_PLANE && u % 16 == 0, "unit of (%d, %d) at %d", d, q, u);
    CHECK(unit_of[u / 16] < 0, "unit %d written twice", u);
    unit_of[u / 16] = d * 4 + q;
    for (int b = 0; b < 16; ++b) { ++owner[u + b]; ++owner[STN_PLANE + u + b]; }
  }
  for (int i = 0; i < (XPIECE - 2 * STN_PLANE) / 4; ++i)
    for (int b = 0; b < 4; ++b) {
      CHECK(2 * STN_PLANE + 4 * i + b < XPIECE, "tail dword %d", i);
      ++owner[2 * STN_PLANE + 4 * i + b];
    }
  for (int b = 0; b < XPIECE; ++b) CHECK(owner[b] == 1, "image byte %d written %d times", b, owner[b]);

  // the DMA of an image: eight waves x five instructions cover every byte, at the same offset in the slot
  for (int slot = 0; slot < 2; ++slot) {
    std::vector<int> got(XPIECE, 0);
    for (int w = 0; w < 8; ++w)
      for (int e = 0; e < 5; ++e) {
        const int I = stn_x_dma_kib(e, w, xkib);
        CHECK(I >= 0 && I < xkib, "KiB %d", I);
        for (int l = 0; l < 64; ++l) {
          const int64_t src = stn_x_dma_src(0, I, l, xkib);
          const int dst = stn_x_dma_lds(slot, I, l, xkib);
          CHECK(src >= 0 && src + 16 <= XPIECE, "image source %lld", (long long)src);
          CHECK(dst >= slot * XPIECE && dst + 16 <= (slot + 1) * XPIECE && dst + 16 <= stn_ring_base(xkib), "image dest %d", dst);
          CHECK(dst - slot * XPIECE == src, "the image is not copied as it is: %d <- %lld", dst, (long long)src);
          CHECK(dst == stn_x_dma_lds(slot, I, 0, xkib) + 16 * l, "lane stride of the DMA");
          for (int b = 0; b < 16; ++b) got[src + b] = 1;
        }
      }
    for (int b = 0; b < XPIECE; ++b) CHECK(got[b] == 1, "image byte %d never copied", b);
  }
  // fragment reads: lane (r, q) of tile j wants column 16 j + r, tokens 8 q ..: the unit the pass wrote for (d, q), in
  // either plane (the kernel adds slot * XPIECE and STN_PLANE to the same offset)
  for (int j = 0; j < STN_NT; ++j)
    for (int r = 0; r < 16; ++r)
      for (int q = 0; q < 4; ++q) {
        const int f = stn_x_frag(j, r, q);
        CHECK(f >= 0 && f + 16 <= STN_PLANE, "fragment %d", f);
        CHECK(f == stn_x_unit(16 * j + r, q) && unit_of[f / 16] == (16 * j + r) * 4 + q, "fragment (%d, %d, %d) reads unit %d", j, r, q, f);
        CHECK(f == stn_x_frag(0, r, q) + 1024 * j, "tile stride of the fragment");
      }
  // ds_read_b128 of the fragments: banks (a / 4) % 64, four groups of sixteen lanes -- every 16-byte slot of the row at most
  // once per group (taken as lanes 16 g .. 16 g + 15 here: one lane quarter, whose sixteen rows x one unit the swizzle
  // spreads over all sixteen slots; the image layout is that of the dx kernel's W image)
  for (int g = 0; g < 4; ++g) {
    int seen[16] = {0};
    for (int l = 16 * g; l < 16 * g + 16; ++l) {
      const int slot16 = (stn_x_frag(0, l & 15, l >> 4) / 16) % 16;
      CHECK(!seen[slot16]++, "fragment read: slot %d twice in group %d", slot16, g);
    }
  }
}

// ---- shape independent: the ring's DMA (source side permuted, LDS side linear) against the transposed read ----------------
static void check_ring(int xkib) {
  const int BASE = stn_ring_base(xkib);
  for (int ring = 0; ring < STN_RING; ++ring) {
    std::vector<int> tok(STN_RAW / 16, -1), chunk(STN_RAW / 16, -1);
    for (int w = 0; w < 8; ++w)
      for (int i = 0; i < 2; ++i) {
        const int I = stn_raw_dma_kib(i, w);
        CHECK(I >= 0 && I < STN_RAWDMA, "KiB %d of the raw piece", I);
        for (int l = 0; l < 64; ++l) {
          const int dst = stn_raw_dma_lds(ring, I, l, xkib);
          CHECK(dst >= BASE + ring * STN_RAW && dst + 16 <= BASE + (ring + 1) * STN_RAW && dst + 16 <= stn_lds(xkib), "ring dest %d", dst);
          CHECK(dst == stn_raw_dma_lds(ring, I, 0, xkib) + 16 * l, "lane stride of the DMA");
          const int t = stn_raw_dma_row(I, l), c = stn_raw_dma_chunk(I, l);
          CHECK(t >= 0 && t < STN_KP && c >= 0 && c < STN_COLS / 4, "row %d chunk %d", t, c);
          const int pos = (dst - BASE - ring * STN_RAW) / 16;
          CHECK(tok[pos] < 0, "ring position %d written twice", pos);
          tok[pos] = t; chunk[pos] = c;
        }
      }
    for (size_t pz = 0; pz < tok.size(); ++pz) CHECK(tok[pz] >= 0, "ring position %zu never written", pz);
    for (int w = 0; w < 8; ++w)
      for (int k = 0; k < 8; ++k)
        for (int half = 0; half < 2; ++half) {
          int bank_seen[32] = {0};
          for (int l = 32 * half; l < 32 * half + 32; ++l) {
            const int r = l & 15, q = l >> 4;
            const int a = stn_raw_read(ring, w, r, q, k, xkib);
            CHECK(a >= BASE + ring * STN_RAW && a + 4 <= BASE + (ring + 1) * STN_RAW, "ring read %d", a);
            CHECK(a == stn_raw_read(0, w, r, q, 0, xkib) + ring * STN_RAW + 512 * k, "token and ring stride of the read");
            const int pos = (a - BASE - ring * STN_RAW) / 16, dw = (a / 4) & 3;
            CHECK(tok[pos] == 8 * q + k, "wave %d lane %d token %d: finds token %d", w, l, 8 * q + k, tok[pos]);
            CHECK(4 * chunk[pos] + dw == 16 * w + r, "wave %d lane %d: finds column %d", w, l, 4 * chunk[pos] + dw);
            CHECK(!bank_seen[(a / 4) % 32]++, "wave %d token %d: bank %d twice in a half", w, k, (a / 4) % 32);   // ds_read_b32: (a / 4) % 32 per 32-lane half
          }
        }
  }
}

// ---- one K range (np pieces from token k_begin) of a raw matrix of `rows` x ncols live floats, rows ld floats apart ----
// Pieces 0 .. np + 2 are asked for (the prologue's four and s + 4 up to s = np - 1); threads take the pieces in turn (a
// piece's 32 rows are whole 64-bit words of the bitmap `fetched`, one bit per live 16-byte chunk).  Then the X images the
// range's waves copy.
static void check_range_fetches(int k_begin, int np, int64_t rows, int ncols, int64_t ld, int xkib, std::vector<uint64_t>& fetched,
                                int64_t* clamped_cols, int64_t* repeats) {
  const int nbx = (ncols + STN_COLS - 1) / STN_COLS, cpr = ncols / 4;
  const int64_t raw_floats = (rows - 1) * ld + ncols;          // the last row need not be padded
  CHECK((32 * (int64_t)cpr) % 64 == 0, "bitmap words straddle pieces");
  const int nthreads = (int)std::thread::hardware_concurrency() >= 8 ? 8 : 2;
  std::vector<int64_t> th_clamped(nthreads, 0), th_repeats(nthreads, 0);
  auto walk = [&](int th) {
    int64_t cl = 0, rp = 0;
    for (int piece = th; piece < np + 3; piece += nthreads)
      for (int bx = 0; bx < nbx; ++bx)
        for (int w = 0; w < 8; ++w)
          for (int i = 0; i < 2; ++i) {
            const int I = stn_raw_dma_kib(i, w);
            for (int l = 0; l < 64; ++l) {
              const int t = stn_raw_dma_row(I, l), c = stn_raw_dma_chunk(I, l);
              const int colc = stn_raw_col(bx, c, ncols);
              const bool real_col = bx * STN_COLS + 4 * c < ncols;
              const int64_t off = stn_raw_src(k_begin, piece, np, t, ld, colc);
              const int64_t row = off / ld;
              // the kernel forms the address as (piece 0's) + min(piece, np - 1) * 32 * ld
              CHECK(off == stn_raw_src(k_begin, 0, 1, t, ld, colc) + (int64_t)stn_min_i(piece, np - 1) * STN_KP * ld, "address split");
              // (one condition: inside the range and the matrix, aligned, an unclamped chunk where it belongs)
              CHECK(row >= k_begin && row < k_begin + (int64_t)np * STN_KP && row < rows && off - row * ld == colc && colc >= 0 &&
                        colc + 4 <= ncols && (off & 3) == 0 && off + 4 <= raw_floats && (!real_col || colc == bx * STN_COLS + 4 * c),
                    "row %lld column %d", (long long)row, colc);
              if (piece >= np) { ++rp; continue; }
              if (!real_col) { ++cl; continue; }
              const int64_t ch = row * cpr + (colc >> 2);
              uint64_t& word = fetched[(size_t)(ch >> 6)];
              const uint64_t bit = 1ull << (ch & 63);
              CHECK(!(word & bit), "chunk (%lld, %d) fetched twice", (long long)row, colc);
              word |= bit;
            }
          }
    th_clamped[th] = cl; th_repeats[th] = rp;
  };
  std::vector<std::thread> pool;
  for (int th = 0; th < nthreads; ++th) pool.emplace_back(walk, th);
  for (int th = 0; th < nthreads; ++th) { pool[th].join(); *clamped_cols += th_clamped[th]; *repeats += th_repeats[th]; }
  // X: pieces 0 .. np - 1 (and the clamped np - 1 once more) of the range, image k_begin / 32 + piece
  const int64_t img_bytes = (rows / STN_KP) * stn_xpiece(xkib);
  for (int w = 0; w < 8; ++w)
    for (int e = 0; e < 5; ++e)
      for (int piece = 0; piece < np; piece += (np > 1 ? np - 1 : 1)) {      // first and last: the offset is linear in between
        const int64_t a = (int64_t)(k_begin / STN_KP) * stn_xpiece(xkib) + stn_x_dma_src(piece, stn_x_dma_kib(e, w, xkib), 63, xkib);
        CHECK(a >= 0 && a + 16 <= img_bytes, "image source %lld of %lld", (long long)a, (long long)img_bytes);
      }
}

// every live chunk of the raw matrix exactly once
static void check_all_fetched(const std::vector<uint64_t>& fetched, int64_t chunks) {
  for (int64_t wd = 0; wd < (chunks + 63) / 64; ++wd) {
    const int64_t left = chunks - wd * 64;
    const uint64_t want = left >= 64 ? ~0ull : (1ull << left) - 1;
    CHECK(fetched[(size_t)wd] == want, "chunks %lld .. %lld: fetched mask %llx", (long long)(wd * 64), (long long)(wd * 64 + 63),
          (unsigned long long)fetched[(size_t)wd]);
  }
}

// the extra region, and the plane pass: block b writes image b from 32 rows of x
static void check_extra_region(int64_t rows, int xkib) {
  const int npieces = (int)(rows / STN_KP);
  const int64_t img_bytes = (int64_t)npieces * stn_xpiece(xkib);
  CHECK(stn_extra_bytes(rows, xkib) == img_bytes + STN_N * 4, "extra region");
  CHECK((int64_t)stn_partials(rows) * STN_N * 4 <= img_bytes, "the partial maxima do not fit the image region");
  for (int b = 0; b < npieces; b += (npieces > 1 ? npieces - 1 : 1)) {
    CHECK((int64_t)(b + 1) * stn_xpiece(xkib) <= img_bytes, "image %d", b);
    for (int k = 0; k < STN_KP; ++k) CHECK((int64_t)b * STN_KP + k < rows, "x row of image %d", b);
  }
}
