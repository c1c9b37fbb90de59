// Host checker of the down-projection weight gradient on the split-fp16 TN pipeline (dW_down^T = g2^T h: the packed kernel of
// pydynet_amd/csrc/outres_tn_split.hip with one block and the TRANSPOSED store) and of the whole-line plane pass
// (pydynet_amd/csrc/split_tn_planes.hip), on pydynet_amd/csrc/split_tn_index.h, the header the kernels use, with the walks of
// tests/split_tn_check.h.  Built with the host compiler and -fsanitize=address,undefined by
// tests/test_down_dw_split_check_cpu.py and run as a process of its own.  For every shape on the command line
// (`K M ldh ldg2`, quadruples: tokens, columns of h = rows of dW_down, row strides of h and of g2) it walks every workgroup,
// wave, lane and piece of the launch and asserts that
//   * every global byte range a DMA, a load or a store forms lies inside its buffer, clamped ones included;
//   * each 16-byte chunk of h's live columns is fetched exactly once, and no byte of a padded row's tail is touched;
//   * every element of every (M x 288) slab is stored exactly once, by 16-byte stores that are aligned, lie inside the slabs
//     in use and hold four consecutive columns of one row of dW_down; no store lands behind the last slab, and the slabs in
//     use stay within the 64 the workspace holds;
// and, shape independent, that the plane pass
//   * loads every 16 bytes of a piece once, inside the piece (padded rows included), and stages them inside its LDS array,
//     every float4 slot written once, 16-byte aligned;
//   * reads back, for unit u of the image, the eight tokens of the column and quarter whose unit stn_x_unit places at byte
//     16 u -- so that the image is what the main kernels' DMA and fragment reads expect (tests/split_tn_check.h) -- with at
//     most two lanes of a wave on one LDS bank;
//   * stores every byte of both planes once, a wave's instruction covering 1 KiB of whole 128-byte lines.
#include "split_tn_check.h"

static void check_pass(int xkib, int64_t ldx) {
  const int XPIECE = stn_xpiece(xkib), NF = STN_KP * STN_N;
  CHECK(NF * 4 <= 64 * 1024, "the staging array leaves a workgroup's LDS");
  std::vector<int> tok(NF, -1), colm(NF, -1);
  std::vector<int> loaded(STN_KP * (STN_N / 4), 0);
  for (int e = 0; e < STN_PASS_LOADS; ++e)
    for (int tid = 0; tid < STN_PASS_THREADS; ++tid) {
      const int i = tid + STN_PASS_THREADS * e, t = stn_pass_row(i), c = stn_pass_chunk(i);
      CHECK(t >= 0 && t < STN_KP && c >= 0 && c < STN_N / 4, "load item %d: row %d chunk %d", i, t, c);
      const int64_t src = (int64_t)t * ldx + 4 * c;
      CHECK(src % 4 == 0 && src + 4 <= (int64_t)(STN_KP - 1) * ldx + STN_N, "load item %d at float %lld", i, (long long)src);
      CHECK(!loaded[t * (STN_N / 4) + c]++, "chunk (%d, %d) loaded twice", t, c);
      const int a = stn_pass_lds(t, 4 * c);
      CHECK(a >= 0 && a + 4 <= NF && a % 4 == 0 && a / STN_N == t, "LDS slot %d of (%d, %d)", a, t, c);
      for (int b = 0; b < 4; ++b) {
        CHECK(stn_pass_lds(t, 4 * c + b) == a + b, "a chunk is not contiguous in LDS");
        CHECK(tok[a + b] < 0, "LDS float %d written twice", a + b);
        tok[a + b] = t; colm[a + b] = 4 * c + b;
      }
    }
  for (int a = 0; a < NF; ++a) CHECK(tok[a] >= 0, "LDS float %d never written", a);
  for (size_t z = 0; z < loaded.size(); ++z) CHECK(loaded[z] == 1, "chunk %zu loaded %d times", z, loaded[z]);

  std::vector<int> owner(XPIECE, 0);
  const int items = (STN_N * 4 + STN_PASS_THREADS - 1) / STN_PASS_THREADS;
  int worst = 0;
  for (int e = 0; e < items; ++e)
    for (int w = 0; w < STN_PASS_THREADS / 64; ++w) {
      int lo = 1 << 30, hi = -1;
      for (int k = 0; k < 8; ++k) {
        int bank[64] = {0};
        for (int l = 0; l < 64; ++l) {
          const int u = 64 * w + l + STN_PASS_THREADS * e;
          if (u >= STN_N * 4) continue;
          const int d = stn_pass_unit_d(u), q = stn_pass_unit_q(u);
          CHECK(d >= 0 && d < STN_N && q >= 0 && q < 4 && stn_x_unit(d, q) == 16 * u, "unit %d is not (%d, %d)", u, d, q);
          const int a = stn_pass_lds(8 * q + k, d);
          CHECK(a >= 0 && a < NF && tok[a] == 8 * q + k && colm[a] == d, "unit %d token %d: finds (%d, %d)", u, 8 * q + k, tok[a], colm[a]);
          const int n = ++bank[a % 64];
          if (n > worst) worst = n;
        }
      }
      for (int l = 0; l < 64; ++l) {
        const int u = 64 * w + l + STN_PASS_THREADS * e;
        if (u >= STN_N * 4) continue;
        CHECK(16 * u + 16 <= STN_PLANE, "unit %d leaves the plane", u);
        for (int b = 0; b < 16; ++b) { ++owner[16 * u + b]; ++owner[STN_PLANE + 16 * u + b]; }
        if (16 * u < lo) lo = 16 * u;
        if (16 * u + 16 > hi) hi = 16 * u + 16;
      }
      if (hi > 0) CHECK(lo % 128 == 0 && hi % 128 == 0 && (hi - lo == 1024 || e == items - 1), "wave %d item %d stores bytes %d .. %d", w, e, lo, hi);
    }
  CHECK(worst <= 2, "%d lanes of a wave on one LDS bank", worst);
  for (int i = 0; i < (XPIECE - 2 * STN_PLANE) / 4; ++i)             // the tail, as before: 256 dwords per KiB
    for (int b = 0; b < 4; ++b) ++owner[2 * STN_PLANE + 4 * i + b];
  for (int b = 0; b < XPIECE; ++b) CHECK(owner[b] == 1, "image byte %d written %d times", b, owner[b]);
  std::printf("plane pass (%d KiB images, ldx %lld): every chunk loaded once, every unit in image order, whole lines, at most %d lanes per bank\n",
              xkib, (long long)ldx, worst);
}

static void check_shape(int K, int M, int64_t ldh, int64_t ldg2) {
  CHECK(K % STN_KP == 0 && K >= OTS_MIN_K && M % 16 == 0 && M >= 512 && M <= 1024 && ldh >= M && ldh % 4 == 0 && ldg2 >= STN_N && ldg2 % 4 == 0,
        "unsupported shape %d x %d, strides %lld, %lld", K, M, (long long)ldh, (long long)ldg2);
  const int npieces = K / STN_KP, nbx = (M + STN_COLS - 1) / STN_COLS;
  const int want = ots_t_ranges(M, npieces);
  const int kps = ots_k_per_split(npieces, want);
  const int ranges = (K + kps - 1) / kps;
  CHECK(want >= 1 && want <= OTS_MAX_RANGES && nbx * want <= 256 && ranges <= want && ranges > 1, "%d ranges of %d column blocks", want, nbx);
  CHECK(kps % STN_KP == 0 && (int64_t)(ranges - 1) * kps < K && (int64_t)ranges * kps >= K, "%d ranges of %d", ranges, kps);
  const int64_t slab = (int64_t)STN_N * M, out_elems = (int64_t)ranges * slab;
  check_extra_region(K, OTS_XKIB);
  check_pass(OTS_XKIB, ldg2);
  CHECK(out_elems <= (int64_t)OTS_MAX_RANGES * slab, "the slabs leave the 64 the workspace holds");

  const int cpr = M / 4;                                       // live 16-byte chunks per row of h
  std::vector<uint64_t> fetched((size_t)(((int64_t)K * cpr + 63) / 64), 0);
  std::vector<uint8_t> stored((size_t)out_elems, 0);
  int64_t clamped_cols = 0, repeats = 0, total_pieces = 0;
  for (int by = 0; by < ranges; ++by) {
    const int k_begin = by * kps, np = stn_range_pieces(K, kps, by);
    CHECK(np >= 1, "range %d is empty", by);
    total_pieces += np;
    check_range_fetches(k_begin, np, K, M, ldh, OTS_XKIB, fetched, &clamped_cols, &repeats);
    for (int bx = 0; bx < nbx; ++bx)
      for (int w = 0; w < 8; ++w) {
        const int c0 = bx * STN_COLS + 16 * w;
        if (c0 >= M) continue;
        CHECK(c0 + 15 < M, "wave at column %d is half used", c0);
        for (int l = 0; l < 64; ++l) {
          const int r = l & 15, q = l >> 4, col = c0 + r;
          for (int j = 0; j < STN_NT; ++j) {
            CHECK(4 * q + 16 * j + 3 < STN_N, "exponent read");
            const int d0 = stn_out_row(j, q, 0);
            const int64_t o = ots_out_elem_t(by, slab, d0, col);
            CHECK(o % 4 == 0 && o >= 0 && o + 4 <= out_elems, "store (%d, %d) at %lld of %lld", col, d0, (long long)o, (long long)out_elems);
            CHECK(o == (int64_t)by * slab + (int64_t)col * STN_N + d0 && d0 + 3 < STN_N, "store (%d, %d) is not row-major in slab %d", col, d0, by);
            for (int i = 0; i < 4; ++i) {
              CHECK(stn_out_row(j, q, i) == d0 + i, "registers of a tile are not consecutive rows");
              CHECK(!stored[o + i]++, "element %lld stored twice", (long long)(o + i));
            }
          }
        }
      }
  }
  CHECK(total_pieces == npieces, "the ranges hold %lld pieces of %d", (long long)total_pieces, npieces);
  check_all_fetched(fetched, (int64_t)K * cpr);
  for (size_t o = 0; o < stored.size(); ++o) CHECK(stored[o] == 1, "slab element %zu stored %d times", o, stored[o]);
  std::printf("K %d rows %d (ldh %lld, ldg2 %lld): %d K ranges of %d tokens, %d column blocks; every h chunk fetched once, "
              "%lld clamped column fetches, %lld repeated fetches behind a range's end; every slab element stored once\n",
              K, M, (long long)ldh, (long long)ldg2, ranges, kps, nbx, (long long)clamped_cols, (long long)repeats);
}

int main(int argc, char** argv) {
  check_x_image(OTS_XKIB);
  check_ring(OTS_XKIB);
  check_pass(LDW_XKIB, STN_N);
  std::printf("layouts: image, DMA, fragment and ring reads agree\n");
  CHECK(argc >= 5 && argc % 4 == 1, "usage: %s K M ldh ldg2 [..]", argv[0]);
  for (int a = 1; a + 3 < argc; a += 4) check_shape(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoll(argv[a + 2]), std::atoll(argv[a + 3]));
  return 0;
}
