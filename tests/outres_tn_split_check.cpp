// Host checker of the split-fp16 packed layer weight gradients' index arithmetic (pydynet_amd/csrc/split_tn_index.h, the
// header the kernels use, through the walks of tests/split_tn_check.h).  Built with the host compiler and
// -fsanitize=address,undefined by tests/test_outres_tn_split_check_cpu.py and run as a process of its own.  For every shape on
// the command line
// (`K nb_cols nbatch ldg`, quadruples) it walks every workgroup, wave, lane and piece of the launch and asserts that
//   * every global byte range a DMA, a load or a store forms lies inside its buffer, clamped ones included;
//   * every LDS offset lies inside the allocation, and inside the region it is meant for;
//   * each 16-byte chunk of g's live columns is fetched exactly once (clamped repeats apart, which are counted), and no
//     byte of a padded row's tail is touched;
//   * every output element is written exactly once, in the block its column belongs to;
//   * what the plane pass writes is what the DMA copies and what the fragment reads address;
//   * the transposed ds_read_b32 of g finds the token and column it wants, free of bank conflicts;
//   * the running exponent keeps g 2^S below 2^15 and only ever falls.
#include <cmath>
#include <cstring>

#include "split_tn_check.h"

// ---- the running exponent: every fp32 magnitude class against every state --------------------------------------------------
static void check_scale() {
  CHECK(ots_next_scale(0u, OTS_S_UNSET) == OTS_S_UNSET && ots_next_scale(0u, 7) == 7, "an all-zero piece changes nothing");
  for (int E = 0; E < 255; ++E)
    for (unsigned man : {0u, 1u, 0x7fffffu}) {
      const unsigned bits = ((unsigned)E << 23) | man;
      if (bits == 0u) continue;
      float v;
      std::memcpy(&v, &bits, 4);
      const int S0 = ots_next_scale(bits, OTS_S_UNSET);
      const double scaled = std::ldexp((double)v, S0);
      CHECK(scaled < 8192.0 && (E == 0 || scaled >= 4096.0), "first exponent %d puts %g at %g", S0, (double)v, scaled);
      for (int S = -120; S <= 139; ++S) {
        const int Sn = ots_next_scale(bits, S);
        const double now = std::ldexp((double)v, S);
        CHECK(Sn <= S, "the exponent rose: %d -> %d", S, Sn);
        if (now < 32768.0) CHECK(Sn == S, "%g 2^%d is below 2^15, yet %d -> %d", (double)v, S, S, Sn);
        else CHECK(Sn < S && std::ldexp((double)v, Sn) < 8192.0 && std::ldexp((double)v, Sn) >= 4096.0, "%g: %d -> %d", (double)v, S, Sn);
      }
    }
}

static void check_shape(int K, int nb_cols, int nbatch, int64_t ldg) {
  const int n_all = nb_cols * nbatch;
  CHECK(K % STN_KP == 0 && K >= OTS_MIN_K && nb_cols % 16 == 0 && nbatch > 1 && n_all >= 768 && n_all <= 8192 && ldg >= n_all && ldg % 4 == 0,
        "unsupported shape %d x (%d x %d), ldg %lld", K, nbatch, nb_cols, (long long)ldg);
  const int npieces = K / STN_KP, nbx = (n_all + STN_COLS - 1) / STN_COLS;
  const int pl = plan(n_all, K);
  const int want = ots_ranges(n_all, pl, npieces);
  const int kps = ots_k_per_split(npieces, want);
  const int ranges = (K + kps - 1) / kps;
  CHECK(want >= (pl < OTS_MAX_RANGES ? pl : OTS_MAX_RANGES) && want <= OTS_MAX_RANGES && ranges <= want && ranges >= 1, "%d ranges against the plan's %d", want, pl);
  CHECK(kps % STN_KP == 0 && (int64_t)(ranges - 1) * kps < K && (int64_t)ranges * kps >= K, "%d ranges of %d", ranges, kps);
  const int64_t slab = (int64_t)STN_N * nb_cols, blk_stride = (int64_t)ranges * slab, out_elems = (int64_t)nbatch * blk_stride;
  check_extra_region(K, OTS_XKIB);
  CHECK(out_elems <= (int64_t)OTS_MAX_RANGES * STN_N * n_all, "the slabs leave the 64 the workspace holds");

  const int cpr = n_all / 4;                                   // live 16-byte chunks per row of g
  std::vector<uint64_t> fetched((size_t)(((int64_t)K * cpr + 63) / 64), 0);
  std::vector<uint8_t> stored((size_t)out_elems, 0);
  int64_t clamped_cols = 0, repeats = 0, total_pieces = 0;

  for (int by = 0; by < ranges; ++by) {
    const int k_begin = by * kps, np = stn_range_pieces(K, kps, by);
    CHECK(np >= 1, "range %d is empty", by);
    total_pieces += np;
    check_range_fetches(k_begin, np, K, n_all, ldg, OTS_XKIB, fetched, &clamped_cols, &repeats);
    for (int bx = 0; bx < nbx; ++bx)
      for (int w = 0; w < 8; ++w) {
        const int c0 = bx * STN_COLS + 16 * w;
        if (c0 >= n_all) continue;                             // the stores of an active wave: sixteen columns of ONE block
        CHECK(c0 / nb_cols == (c0 + 15) / nb_cols && c0 + 15 < n_all, "wave at column %d straddles two blocks", c0);
        for (int l = 0; l < 64; ++l) {
          const int r = l & 15, q = l >> 4, col = c0 + r;
          for (int j = 0; j < STN_NT; ++j) {
            CHECK(4 * q + 16 * j + 3 < STN_N, "exponent read");
            for (int i = 0; i < 4; ++i) {
              const int d = stn_out_row(j, q, i);
              const int64_t o = ots_out_elem(by, slab, blk_stride, nb_cols, d, col);
              const int b = col / nb_cols;
              CHECK(d >= 0 && d < STN_N && o >= 0 && o < out_elems, "store (%d, %d) at %lld", d, col, (long long)o);
              CHECK(o == ((int64_t)b * ranges + by) * slab + (int64_t)d * nb_cols + (col - b * nb_cols), "store (%d, %d) not in block %d", d, col, b);
              CHECK(!stored[o]++, "element %lld stored twice", (long long)o);
            }
          }
        }
      }
  }
  CHECK(total_pieces == npieces, "the ranges hold %lld pieces of %d", (long long)total_pieces, npieces);
  check_all_fetched(fetched, (int64_t)K * cpr);
  for (size_t o = 0; o < stored.size(); ++o) CHECK(stored[o] == 1, "slab element %zu stored %d times", o, stored[o]);
  std::printf("K %d columns %d x %d (ldg %lld): %d K ranges of %d tokens (plan %d), %d column blocks; every g chunk fetched once, "
              "%lld clamped column fetches, %lld repeated fetches behind a range's end; every slab element stored once\n",
              K, nbatch, nb_cols, (long long)ldg, ranges, kps, pl, nbx, (long long)clamped_cols, (long long)repeats);
}

int main(int argc, char** argv) {
  check_x_image(OTS_XKIB);
  check_ring(OTS_XKIB);
  std::printf("layouts: image, DMA, fragment and ring reads agree; transposed read free of bank conflicts\n");
  check_scale();
  std::printf("running exponent: below 2^15, only ever falls\n");
  CHECK(argc >= 5 && argc % 4 == 1, "usage: %s K nb_cols nbatch ldg [..]", argv[0]);
  for (int a = 1; a + 3 < argc; a += 4) check_shape(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), std::atoll(argv[a + 3]));
  return 0;
}
