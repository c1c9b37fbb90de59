// Host checker of the split-fp16 lm_head weight gradient's index arithmetic (pydynet_amd/csrc/lm_head_dw_split_index.h,
// the header the kernels use).  Built with the host compiler and -fsanitize=address,undefined by
// tests/test_lm_head_dw_split_check_cpu.py and run as a process of its own.  For every shape on the command line
// (`rows V`, pairs) it walks every workgroup, wave, lane and piece of the launch and asserts that
//   * every global byte range a DMA, a load or a store forms lies inside its buffer, clamped ones included;
//   * every LDS offset lies inside the allocation, and inside the region it is meant for;
//   * each 16-byte chunk of the logits matrix is fetched exactly once (clamped repeats apart, which are counted);
//   * what the plane pass writes is what the DMA copies and what the fragment / tail reads address;
//   * the transposed ds_read_b32 of the logits finds the token and column it wants, free of bank conflicts.
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../pydynet_amd/csrc/lm_head_dw_split_index.h"

#define CHECK(c, ...)                                                                     \
  do {                                                                                    \
    if (!(c)) {                                                                           \
      std::fprintf(stderr, "CHECK failed at line %d: %s\n  ", __LINE__, #c);              \
      std::fprintf(stderr, __VA_ARGS__);                                                  \
      std::fprintf(stderr, "\n");                                                         \
      std::fflush(stderr);                                                                \
      std::_Exit(1);                                                                      \
    }                                                                                     \
  } while (0)

// the K ranges of the fp32 kernel (pdn_gemm_outres_tn_plan of csrc/gemm_outres.hip at its default of eight waves)
static int plan(int N, int K, int* kps_out) {
  const int col_wgs = (N / 32 + 7) / 8;
  int splits = 256 / (col_wgs > 0 ? col_wgs : 1);
  if (splits < 1) splits = 1;
  if (splits >= 16 && col_wgs > 1) splits &= ~7;
  const int pieces = K / 32;
  if (splits > pieces) splits = pieces > 0 ? pieces : 1;
  const int kps = ((pieces + splits - 1) / splits) * 32;
  *kps_out = kps;
  return (K + kps - 1) / kps;
}

// ---- shape independent: the image, its DMA, the fragment reads; the ring's DMA against its transposed read -----------
static void check_layouts() {
  // plane pass: thread item i -> (d, q) -> two units; the tail: 256 dwords
  std::vector<int> owner(LDW_XPIECE, 0);
  std::vector<int> unit_of(LDW_PLANE / 16, -1);
  for (int i = 0; i < LDW_N * 4; ++i) {
    const int d = i % LDW_N, q = i / LDW_N, u = ldw_x_unit(d, q);
    CHECK(u >= 0 && u + 16 <= LDW_PLANE && u % 16 == 0, "unit of (%d, %d) at %d", d, q, u);
    CHECK(unit_of[u / 16] < 0, "unit %d written twice", u);
    unit_of[u / 16] = d * 4 + q;
    for (int b = 0; b < 16; ++b) { ++owner[u + b]; ++owner[LDW_PLANE + u + b]; }
  }
  for (int i = 0; i < 256; ++i)
    for (int b = 0; b < 4; ++b) {
      CHECK(LDW_TAIL + 4 * i + b < LDW_XPIECE, "tail dword %d", i);
      ++owner[LDW_TAIL + 4 * i + b];
    }
  for (int b = 0; b < LDW_XPIECE; ++b) CHECK(owner[b] == 1, "image byte %d written %d times", b, owner[b]);

  // the DMA of an image: eight waves x five instructions cover every byte, at the same offset in the slot
  for (int slot = 0; slot < 2; ++slot) {
    std::vector<int> got(LDW_XPIECE, 0);
    for (int w = 0; w < 8; ++w)
      for (int e = 0; e < 5; ++e) {
        const int I = ldw_x_dma_kib(e, w);
        CHECK(I >= 0 && I < LDW_XDMA, "KiB %d", I);
        for (int l = 0; l < 64; ++l) {
          const int64_t src = ldw_x_dma_src(0, I, l);
          const int dst = ldw_x_dma_lds(slot, I, l);
          CHECK(src >= 0 && src + 16 <= LDW_XPIECE, "image source %lld", (long long)src);
          CHECK(dst >= slot * LDW_XPIECE && dst + 16 <= (slot + 1) * LDW_XPIECE && dst + 16 <= LDW_RING_BASE, "image dest %d", dst);
          CHECK(dst - slot * LDW_XPIECE == src, "the image is not copied as it is: %d <- %lld", dst, (long long)src);
          CHECK(dst == ldw_x_dma_lds(slot, I, 0) + 16 * l, "lane stride of the DMA");
          for (int b = 0; b < 16; ++b) got[src + b] = 1;
        }
      }
    for (int b = 0; b < LDW_XPIECE; ++b) CHECK(got[b] == 1, "image byte %d never copied", b);
  }
  // fragment reads: lane (r, q) of tile j wants column 16 j + r, tokens 8 q ..: the unit the pass wrote for (d, q)
  for (int j = 0; j < LDW_NT; ++j)
    for (int r = 0; r < 16; ++r)
      for (int q = 0; q < 4; ++q) {
        const int f = ldw_x_frag(j, r, q);
        CHECK(f >= 0 && f + 16 <= LDW_PLANE, "fragment %d", f);
        CHECK(f == ldw_x_unit(16 * j + r, q) && unit_of[f / 16] == (16 * j + r) * 4 + q, "fragment (%d, %d, %d) reads unit %d", j, r, q, f);
      }
  // ds_read_b128 of the fragments: banks (a / 4) % 64, four groups of sixteen lanes -- every 16-byte slot of the row at most
  // once per group (taken as lanes 16 g .. 16 g + 15 here: one lane quarter, whose sixteen rows x one unit the swizzle
  // spreads over all sixteen slots; the image layout is that of the dx kernel's W image)
  for (int g = 0; g < 4; ++g) {
    int seen[16] = {0};
    for (int l = 16 * g; l < 16 * g + 16; ++l) {
      const int slot16 = (ldw_x_frag(0, l & 15, l >> 4) / 16) % 16;
      CHECK(!seen[slot16]++, "fragment read: slot %d twice in group %d", slot16, g);
    }
  }
  // tail reads
  for (int slot = 0; slot < 2; ++slot)
    for (int t = 0; t < 32; ++t) {
      const int a = ldw_tail_nl(slot, t), b = ldw_tail_tg(slot, t);
      CHECK(a >= slot * LDW_XPIECE + LDW_TAIL && a + 4 <= slot * LDW_XPIECE + LDW_TAIL + 128, "tail lse %d", a);
      CHECK(b >= slot * LDW_XPIECE + LDW_TAIL + 128 && b + 4 <= slot * LDW_XPIECE + LDW_TAIL + 256, "tail target %d", b);
    }

  // the ring: DMA (source side permuted, LDS side linear) against the transposed read
  for (int ring = 0; ring < LDW_RING; ++ring) {
    std::vector<int> tok(LDW_RAW / 16, -1), chunk(LDW_RAW / 16, -1);
    for (int w = 0; w < 8; ++w)
      for (int i = 0; i < 2; ++i) {
        const int I = ldw_raw_dma_kib(i, w);
        CHECK(I >= 0 && I < LDW_RAWDMA, "KiB %d of the logits", I);
        for (int l = 0; l < 64; ++l) {
          const int dst = ldw_raw_dma_lds(ring, I, l);
          CHECK(dst >= LDW_RING_BASE + ring * LDW_RAW && dst + 16 <= LDW_RING_BASE + (ring + 1) * LDW_RAW && dst + 16 <= LDW_LDS, "ring dest %d", dst);
          CHECK(dst == ldw_raw_dma_lds(ring, I, 0) + 16 * l, "lane stride of the DMA");
          const int t = ldw_raw_dma_row(I, l), c = ldw_raw_dma_chunk(I, l);
          CHECK(t >= 0 && t < LDW_KP && c >= 0 && c < LDW_COLS / 4, "row %d chunk %d", t, c);
          const int pos = (dst - LDW_RING_BASE - ring * LDW_RAW) / 16;
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
            const int a = ldw_raw_read(ring, w, r, q, k);
            CHECK(a >= LDW_RING_BASE + ring * LDW_RAW && a + 4 <= LDW_RING_BASE + (ring + 1) * LDW_RAW, "ring read %d", a);
            CHECK(a == ldw_raw_read(ring, w, r, q, 0) + 512 * k, "token stride of the read");
            const int pos = (a - LDW_RING_BASE - ring * LDW_RAW) / 16, dw = (a / 4) & 3;
            CHECK(tok[pos] == 8 * q + k, "wave %d lane %d token %d: finds token %d", w, l, 8 * q + k, tok[pos]);
            CHECK(4 * chunk[pos] + dw == 16 * w + r, "wave %d lane %d: finds column %d", w, l, 4 * chunk[pos] + dw);
            CHECK(!bank_seen[(a / 4) % 32]++, "wave %d token %d: bank %d twice in a half", w, k, (a / 4) % 32);   // ds_read_b32: (a / 4) % 32 per 32-lane half
          }
        }
  }
  static_assert(LDW_LDS <= 160 * 1024, "LDS allocation");
  static_assert(LDW_RING_BASE % 1024 == 0 && LDW_XPIECE % 1024 == 0 && LDW_RAW % 1024 == 0, "DMA granularity");
}

static void check_shape(int64_t rows, int V) {
  CHECK(rows % LDW_KP == 0 && rows >= LDW_MIN_ROWS && V % 32 == 0 && V >= LDW_MIN_V, "unsupported shape %lld x %d", (long long)rows, V);
  int kps;
  const int splits = plan(V, (int)rows, &kps);
  const int K = (int)rows, npieces = K / LDW_KP, nbx = (V + LDW_COLS - 1) / LDW_COLS;
  const int64_t logit_bytes = rows * V * 4, slab = (int64_t)LDW_N * V;
  const int64_t img_bytes = (int64_t)npieces * LDW_XPIECE, extra = ldw_extra_bytes(rows);
  CHECK(extra == img_bytes + LDW_N * 4, "extra region");
  CHECK((int64_t)ldw_partials(rows) * LDW_N * 4 <= img_bytes, "the partial maxima do not fit the image region");
  CHECK(kps % LDW_KP == 0 && (int64_t)(splits - 1) * kps < rows && (int64_t)splits * kps >= rows, "plan: %d ranges of %d", splits, kps);

  const int cpr = V / 4;                                       // 16-byte chunks per row of logits
  std::vector<uint64_t> fetched((size_t)((rows * cpr + 63) / 64), 0);
  std::vector<uint8_t> stored((size_t)splits * slab, 0);
  std::vector<uint8_t> cs_stored((size_t)splits * V, 0);
  int64_t clamped_cols = 0, repeats = 0, total_pieces = 0;

  for (int by = 0; by < splits; ++by) {
    const int k_begin = by * kps, np = ldw_range_pieces(K, kps, by);
    CHECK(np >= 1, "range %d is empty", by);
    total_pieces += np;
    // prologue statistics and the plane pass's tails
    for (int q = 0; q < 4; ++q)
      for (int k = 0; k < 8; ++k) CHECK(k_begin + 8 * q + k < rows, "prologue row");
    // logits: pieces 0 .. np + 2 are asked for (the prologue's four and s + 4 up to s = np - 1); piece-major, so that the
    // bitmap is walked in memory order
    // (threads take the pieces in turn: a piece's 32 rows are whole 64-bit words of the bitmap, as 32 V / 4 chunks are)
    CHECK((32 * (int64_t)cpr) % 64 == 0, "bitmap words straddle pieces");
    const int nthreads = (int)std::thread::hardware_concurrency() >= 8 ? 8 : 2;
    std::vector<int64_t> th_clamped(nthreads, 0), th_repeats(nthreads, 0);
    auto walk = [&](int th) {
      int64_t clamped_cols = 0, repeats = 0;
    for (int piece = th; piece < np + 3; piece += nthreads)
      for (int bx = 0; bx < nbx; ++bx)
        for (int w = 0; w < 8; ++w)
          for (int i = 0; i < 2; ++i) {
            const int I = ldw_raw_dma_kib(i, w);
            for (int l = 0; l < 64; ++l) {
              const int t = ldw_raw_dma_row(I, l), c = ldw_raw_dma_chunk(I, l);
              const int colc = ldw_raw_col(bx, c, V);
              const bool real_col = bx * LDW_COLS + 4 * c < V;
              const int64_t row = ldw_raw_row(k_begin, piece, np, t);
              const int64_t byte = (row * V + colc) * 4;
              // (one condition: inside the range and the matrix, aligned, an unclamped chunk where it belongs)
              CHECK(row >= k_begin && row < k_begin + (int64_t)np * LDW_KP && row < rows && colc >= 0 && colc + 4 <= V &&
                        (byte & 15) == 0 && byte + 16 <= logit_bytes && (!real_col || colc == bx * LDW_COLS + 4 * c),
                    "row %lld column %d", (long long)row, colc);
              if (piece >= np) { ++repeats; continue; }
              if (!real_col) { ++clamped_cols; continue; }
              const int64_t ch = row * cpr + (colc >> 2);
              uint64_t& word = fetched[(size_t)(ch >> 6)];
              const uint64_t bit = 1ull << (ch & 63);
              CHECK(!(word & bit), "chunk (%lld, %d) fetched twice", (long long)row, colc);
              word |= bit;
            }
          }
      th_clamped[th] = clamped_cols; th_repeats[th] = repeats;
    };
    std::vector<std::thread> pool;
    for (int th = 0; th < nthreads; ++th) pool.emplace_back(walk, th);
    for (int th = 0; th < nthreads; ++th) { pool[th].join(); clamped_cols += th_clamped[th]; repeats += th_repeats[th]; }
    for (int bx = 0; bx < nbx; ++bx)
      for (int w = 0; w < 8; ++w) {
        const int c0 = bx * LDW_COLS + 16 * w;
        // X: pieces 0 .. np - 1 (and the clamped np - 1 once more) of the range, image k_begin / 32 + piece
        for (int e = 0; e < 5; ++e)
          for (int piece = 0; piece < np; piece += (np > 1 ? np - 1 : 1)) {      // first and last: the offset is linear in between
            const int64_t a = (int64_t)(k_begin / LDW_KP) * LDW_XPIECE + ldw_x_dma_src(piece, ldw_x_dma_kib(e, w), 63);
            CHECK(a >= 0 && a + 16 <= img_bytes, "image source %lld of %lld", (long long)a, (long long)img_bytes);
          }
        // the stores of an active wave
        if (c0 >= V) continue;
        for (int l = 0; l < 64; ++l) {
          const int r = l & 15, q = l >> 4, col = c0 + r;
          CHECK(col < V, "column %d of an active wave", col);
          if (q == 0) {
            const int64_t o = (int64_t)by * V + col;
            CHECK(o >= 0 && o < (int64_t)splits * V && !cs_stored[o]++, "column sum %lld", (long long)o);
          }
          for (int j = 0; j < LDW_NT; ++j) {
            CHECK(4 * q + 16 * j + 3 < LDW_N, "exponent read");
            for (int i = 0; i < 4; ++i) {
              const int d = ldw_out_row(j, q, i);
              const int64_t o = ldw_out_elem(by, slab, d, V, col);
              CHECK(d >= 0 && d < LDW_N && o >= 0 && o < (int64_t)splits * slab, "store (%d, %d) at %lld", d, col, (long long)o);
              CHECK(!stored[o]++, "element %lld stored twice", (long long)o);
            }
          }
        }
      }
  }
  CHECK(total_pieces == npieces, "the ranges hold %lld pieces of %d", (long long)total_pieces, npieces);
  for (int64_t wd = 0; wd < (rows * cpr + 63) / 64; ++wd) {
    const int64_t left = rows * cpr - wd * 64;
    const uint64_t want = left >= 64 ? ~0ull : (1ull << left) - 1;
    CHECK(fetched[(size_t)wd] == want, "chunks %lld .. %lld: fetched mask %llx", (long long)(wd * 64), (long long)(wd * 64 + 63),
          (unsigned long long)fetched[(size_t)wd]);
  }
  for (size_t o = 0; o < stored.size(); ++o) CHECK(stored[o] == 1, "slab element %zu stored %d times", o, stored[o]);
  for (size_t o = 0; o < cs_stored.size(); ++o) CHECK(cs_stored[o] == 1, "column sum %zu stored %d times", o, cs_stored[o]);
  // the plane pass: block b writes image b; its tail reads lse / targets of piece b + 1 only where that exists
  for (int b = 0; b < npieces; b += (npieces > 1 ? npieces - 1 : 1)) {
    CHECK((int64_t)(b + 1) * LDW_XPIECE <= img_bytes, "image %d", b);
    for (int k = 0; k < LDW_KP; ++k) CHECK((int64_t)b * LDW_KP + k < rows, "x row of image %d", b);
  }
  std::printf("rows %lld V %d: %d K ranges of %d tokens, %d column blocks; every logits chunk fetched once, %lld clamped column fetches, "
              "%lld repeated fetches behind a range's end; slabs and column sums stored once\n",
              (long long)rows, V, splits, kps, nbx, (long long)clamped_cols, (long long)repeats);
}

int main(int argc, char** argv) {
  check_layouts();
  std::printf("layouts: image, DMA, fragment, tail and ring reads agree; transposed read free of bank conflicts\n");
  CHECK(argc >= 3 && argc % 2 == 1, "usage: %s rows V [rows V ..]", argv[0]);
  for (int a = 1; a + 1 < argc; a += 2) check_shape(std::atoll(argv[a]), std::atoi(argv[a + 1]));
  return 0;
}
