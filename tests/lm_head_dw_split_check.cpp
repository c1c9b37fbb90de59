// Host checker of the split-fp16 lm_head weight gradient's index arithmetic (pydynet_amd/csrc/split_tn_index.h, the header
// the kernels use, through the walks of tests/split_tn_check.h).  Built with the host compiler and
// -fsanitize=address,undefined by tests/test_lm_head_dw_split_check_cpu.py and run as a process of its own.  For every
// shape on the command line (`rows V`, pairs) it walks every workgroup, wave, lane and piece of the launch and asserts that
//   * every global byte range a DMA, a load or a store forms lies inside its buffer, clamped ones included;
//   * every LDS offset lies inside the allocation, and inside the region it is meant for;
//   * each 16-byte chunk of the logits matrix is fetched exactly once (clamped repeats apart, which are counted);
//   * what the plane pass writes is what the DMA copies and what the fragment / tail reads address;
//   * the transposed ds_read_b32 of the logits finds the token and column it wants, free of bank conflicts.
#include "split_tn_check.h"

static void check_tail() {
  const int XPIECE = stn_xpiece(LDW_XKIB);
  for (int slot = 0; slot < 2; ++slot)
    for (int t = 0; t < 32; ++t) {
      const int a = ldw_tail_nl(slot, t), b = ldw_tail_tg(slot, t);
      CHECK(a >= slot * XPIECE + LDW_TAIL && a + 4 <= slot * XPIECE + LDW_TAIL + 128, "tail lse %d", a);
      CHECK(b >= slot * XPIECE + LDW_TAIL + 128 && b + 4 <= slot * XPIECE + LDW_TAIL + 256, "tail target %d", b);
    }
}

static void check_shape(int64_t rows, int V) {
  CHECK(rows % STN_KP == 0 && rows >= LDW_MIN_ROWS && V % 32 == 0 && V >= LDW_MIN_V, "unsupported shape %lld x %d", (long long)rows, V);
  int kps;
  const int splits = plan(V, (int)rows, &kps);
  const int K = (int)rows, npieces = K / STN_KP, nbx = (V + STN_COLS - 1) / STN_COLS;
  const int64_t slab = (int64_t)STN_N * V;
  check_extra_region(rows, LDW_XKIB);
  CHECK(kps % STN_KP == 0 && (int64_t)(splits - 1) * kps < rows && (int64_t)splits * kps >= rows, "plan: %d ranges of %d", splits, kps);

  const int cpr = V / 4;                                       // 16-byte chunks per row of logits
  std::vector<uint64_t> fetched((size_t)((rows * cpr + 63) / 64), 0);
  std::vector<uint8_t> stored((size_t)splits * slab, 0);
  std::vector<uint8_t> cs_stored((size_t)splits * V, 0);
  int64_t clamped_cols = 0, repeats = 0, total_pieces = 0;

  for (int by = 0; by < splits; ++by) {
    const int k_begin = by * kps, np = stn_range_pieces(K, kps, by);
    CHECK(np >= 1, "range %d is empty", by);
    total_pieces += np;
    // prologue statistics (the plane pass's tails hold those of the later pieces)
    for (int q = 0; q < 4; ++q)
      for (int k = 0; k < 8; ++k) CHECK(k_begin + 8 * q + k < rows, "prologue row");
    check_range_fetches(k_begin, np, rows, V, V, LDW_XKIB, fetched, &clamped_cols, &repeats);
    for (int bx = 0; bx < nbx; ++bx)
      for (int w = 0; w < 8; ++w) {
        const int c0 = bx * STN_COLS + 16 * w;
        if (c0 >= V) continue;                                 // the stores of an active wave
        for (int l = 0; l < 64; ++l) {
          const int r = l & 15, q = l >> 4, col = c0 + r;
          CHECK(col < V, "column %d of an active wave", col);
          if (q == 0) {
            const int64_t o = (int64_t)by * V + col;
            CHECK(o >= 0 && o < (int64_t)splits * V && !cs_stored[o]++, "column sum %lld", (long long)o);
          }
          for (int j = 0; j < STN_NT; ++j) {
            CHECK(4 * q + 16 * j + 3 < STN_N, "exponent read");
            for (int i = 0; i < 4; ++i) {
              const int d = stn_out_row(j, q, i);
              const int64_t o = ldw_out_elem(by, slab, d, V, col);
              CHECK(d >= 0 && d < STN_N && o >= 0 && o < (int64_t)splits * slab, "store (%d, %d) at %lld", d, col, (long long)o);
              CHECK(!stored[o]++, "element %lld stored twice", (long long)o);
            }
          }
        }
      }
  }
  CHECK(total_pieces == npieces, "the ranges hold %lld pieces of %d", (long long)total_pieces, npieces);
  check_all_fetched(fetched, rows * cpr);
  for (size_t o = 0; o < stored.size(); ++o) CHECK(stored[o] == 1, "slab element %zu stored %d times", o, stored[o]);
  for (size_t o = 0; o < cs_stored.size(); ++o) CHECK(cs_stored[o] == 1, "column sum %zu stored %d times", o, cs_stored[o]);
  std::printf("rows %lld V %d: %d K ranges of %d tokens, %d column blocks; every logits chunk fetched once, %lld clamped column fetches, "
              "%lld repeated fetches behind a range's end; slabs and column sums stored once\n",
              (long long)rows, V, splits, kps, nbx, (long long)clamped_cols, (long long)repeats);
}

int main(int argc, char** argv) {
  check_x_image(LDW_XKIB);
  check_tail();
  check_ring(LDW_XKIB);
  std::printf("layouts: image, DMA, fragment, tail and ring reads agree; transposed read free of bank conflicts\n");
  CHECK(argc >= 3 && argc % 2 == 1, "usage: %s rows V [rows V ..]", argv[0]);
  for (int a = 1; a + 1 < argc; a += 2) check_shape(std::atoll(argv[a]), std::atoi(argv[a + 1]));
  return 0;
}
