// Host checker of the split-fp16 packed layer weight gradients' index arithmetic (pydynet_amd/csrc/outres_tn_split_index.h,
// the header the kernels use).  Built with the host compiler and -fsanitize=address,undefined by
// tests/test_outres_tn_split_check_cpu.py and run as a process of its own.  For every shape on the command line
// (`K nb_cols nbatch ldg`, quadruples) it walks every workgroup, wave, lane and piece of the launch and asserts that
//   * every global byte range a DMA, a load or a store forms lies inside its buffer, clamped ones included;
//   * every LDS offset lies inside the allocation, and inside the region it is meant for;
//   * each 16-byte chunk of g's live columns is fetched exactly once (clamped repeats apart, which are counted), and no
//     byte of a padded row's tail is touched;
//   * every output element is written exactly once, in the block its column belongs to;
//   * what the plane pass writes is what the DMA copies and what the fragment reads address;
//   * the transposed ds_read_b32 of g finds the token and column it wants, free of bank conflicts;
//   * the running exponent keeps g 2^S below 2^15 and only ever falls.
#include <cassert>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../pydynet_amd/csrc/outres_tn_split_index.h"

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
static int plan(int N, int K) {
  const int col_wgs = (N / 32 + 7) / 8;
  int splits = 256 / (col_wgs > 0 ? col_wgs : 1);
  if (splits < 1) splits = 1;
  if (splits >= 16 && col_wgs > 1) splits &= ~7;
  const int pieces = K / 32;
  if (splits > pieces) splits = pieces > 0 ? pieces : 1;
  const int kps = ((pieces + splits - 1) / splits) * 32;
  return (K + kps - 1) / kps;
}

// ---- shape independent: the image, its DMA, the fragment reads; the ring's DMA against its transposed read -----------
static void check_layouts() {
  static_assert(OTS_XPIECE == 2 * LDW_PLANE, "an image is two planes");
  static_assert(OTS_LDS <= 160 * 1024, "LDS allocation");
  static_assert(OTS_RING_BASE % 1024 == 0 && OTS_XPIECE % 1024 == 0 && OTS_RAW % 1024 == 0, "DMA granularity");
  // plane pass: thread item i -> (d, q) -> two units
  std::vector<int> owner(OTS_XPIECE, 0);
  std::vector<int> unit_of(LDW_PLANE / 16, -1);
  for (int i = 0; i < LDW_N * 4; ++i) {
    const int d = i % LDW_N, q = i / LDW_N, u = ldw_x_unit(d, q);
    CHECK(u >= 0 && u + 16 <= LDW_PLANE && u % 16 == 0, "unit of (%d, %d) at %d", d, q, u);
    CHECK(unit_of[u / 16] < 0, "unit %d written twice", u);
    unit_of[u / 16] = d * 4 + q;
    for (int b = 0; b < 16; ++b) { ++owner[u + b]; ++owner[LDW_PLANE + u + b]; }
  }
  for (int b = 0; b < OTS_XPIECE; ++b) CHECK(owner[b] == 1, "image byte %d written %d times", b, owner[b]);

  // the DMA of an image: eight waves x five instructions cover every byte, at the same offset in the slot
  for (int slot = 0; slot < 2; ++slot) {
    std::vector<int> got(OTS_XPIECE, 0);
    for (int w = 0; w < 8; ++w)
      for (int e = 0; e < 5; ++e) {
        const int I = ots_x_dma_kib(e, w);
        CHECK(I >= 0 && I < OTS_XDMA, "KiB %d", I);
        for (int l = 0; l < 64; ++l) {
          const int64_t src = ots_x_dma_src(0, I, l);
          const int dst = ots_x_dma_lds(slot, I, l);
          CHECK(src >= 0 && src + 16 <= OTS_XPIECE, "image source %lld", (long long)src);
          CHECK(dst >= slot * OTS_XPIECE && dst + 16 <= (slot + 1) * OTS_XPIECE && dst + 16 <= OTS_RING_BASE, "image dest %d", dst);
          CHECK(dst - slot * OTS_XPIECE == src, "the image is not copied as it is: %d <- %lld", dst, (long long)src);
          CHECK(dst == ots_x_dma_lds(slot, I, 0) + 16 * l, "lane stride of the DMA");
          for (int b = 0; b < 16; ++b) got[src + b] = 1;
        }
      }
    for (int b = 0; b < OTS_XPIECE; ++b) CHECK(got[b] == 1, "image byte %d never copied", b);
    // fragment reads: lane (r, q) of tile j wants column 16 j + r, tokens 8 q ..: the unit the pass wrote for (d, q)
    for (int plane = 0; plane < 2; ++plane)
      for (int j = 0; j < LDW_NT; ++j)
        for (int r = 0; r < 16; ++r)
          for (int q = 0; q < 4; ++q) {
            const int f = ots_x_frag(slot, j, r, q, plane) - slot * OTS_XPIECE - plane * LDW_PLANE;
            CHECK(f >= 0 && f + 16 <= LDW_PLANE, "fragment %d", f);
            CHECK(f == ldw_x_unit(16 * j + r, q) && unit_of[f / 16] == (16 * j + r) * 4 + q, "fragment (%d, %d, %d) reads unit %d", j, r, q, f);
            CHECK(f == ldw_x_frag(0, r, q) + 1024 * j, "tile stride of the fragment");
          }
  }
  // ds_read_b128 of the fragments: every 16-byte slot of a 256-byte row at most once per group of sixteen lanes
  for (int g = 0; g < 4; ++g) {
    int seen[16] = {0};
    for (int l = 16 * g; l < 16 * g + 16; ++l) {
      const int slot16 = (ldw_x_frag(0, l & 15, l >> 4) / 16) % 16;
      CHECK(!seen[slot16]++, "fragment read: slot %d twice in group %d", slot16, g);
    }
  }

  // the ring: DMA (source side permuted, LDS side linear) against the transposed read
  for (int ring = 0; ring < OTS_RING; ++ring) {
    std::vector<int> tok(OTS_RAW / 16, -1), chunk(OTS_RAW / 16, -1);
    for (int w = 0; w < 8; ++w)
      for (int i = 0; i < 2; ++i) {
        const int I = ots_g_dma_kib(i, w);
        CHECK(I >= 0 && I < LDW_RAWDMA, "KiB %d of g", I);
        for (int l = 0; l < 64; ++l) {
          const int dst = ots_g_dma_lds(ring, I, l);
          CHECK(dst >= OTS_RING_BASE + ring * OTS_RAW && dst + 16 <= OTS_RING_BASE + (ring + 1) * OTS_RAW && dst + 16 <= OTS_LDS, "ring dest %d", dst);
          CHECK(dst == ots_g_dma_lds(ring, I, 0) + 16 * l, "lane stride of the DMA");
          const int t = ots_g_dma_row(I, l), c = ots_g_dma_chunk(I, l);
          CHECK(t >= 0 && t < LDW_KP && c >= 0 && c < OTS_COLS / 4, "row %d chunk %d", t, c);
          const int pos = (dst - OTS_RING_BASE - ring * OTS_RAW) / 16;
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
            const int a = ots_g_read(ring, w, r, q, k);
            CHECK(a >= OTS_RING_BASE + ring * OTS_RAW && a + 4 <= OTS_RING_BASE + (ring + 1) * OTS_RAW, "ring read %d", a);
            CHECK(a == ots_g_read(0, w, r, q, 0) + ring * OTS_RAW + 512 * k, "token and ring stride of the read");
            const int pos = (a - OTS_RING_BASE - ring * OTS_RAW) / 16, dw = (a / 4) & 3;
            CHECK(tok[pos] == 8 * q + k, "wave %d lane %d token %d: finds token %d", w, l, 8 * q + k, tok[pos]);
            CHECK(4 * chunk[pos] + dw == 16 * w + r, "wave %d lane %d: finds column %d", w, l, 4 * chunk[pos] + dw);
            CHECK(!bank_seen[(a / 4) % 32]++, "wave %d token %d: bank %d twice in a half", w, k, (a / 4) % 32);   // ds_read_b32: (a / 4) % 32 per 32-lane half
          }
        }
  }
}

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
  CHECK(K % LDW_KP == 0 && K >= OTS_MIN_K && nb_cols % 16 == 0 && nbatch > 1 && n_all >= 768 && n_all <= 8192 && ldg >= n_all && ldg % 4 == 0,
        "unsupported shape %d x (%d x %d), ldg %lld", K, nbatch, nb_cols, (long long)ldg);
  const int npieces = K / LDW_KP, nbx = (n_all + OTS_COLS - 1) / OTS_COLS;
  const int pl = plan(n_all, K);
  const int want = ots_ranges(n_all, pl, npieces);
  const int kps = ots_k_per_split(npieces, want);
  const int ranges = (K + kps - 1) / kps;
  CHECK(want >= (pl < OTS_MAX_RANGES ? pl : OTS_MAX_RANGES) && want <= OTS_MAX_RANGES && ranges <= want && ranges >= 1, "%d ranges against the plan's %d", want, pl);
  CHECK(kps % LDW_KP == 0 && (int64_t)(ranges - 1) * kps < K && (int64_t)ranges * kps >= K, "%d ranges of %d", ranges, kps);
  const int64_t g_floats = (int64_t)(K - 1) * ldg + n_all;      // the last row need not be padded
  const int64_t slab = (int64_t)LDW_N * nb_cols, blk_stride = (int64_t)ranges * slab, out_elems = (int64_t)nbatch * blk_stride;
  const int64_t img_bytes = (int64_t)npieces * OTS_XPIECE, extra = ots_extra_bytes(K);
  CHECK(extra == img_bytes + LDW_N * 4, "extra region");
  CHECK((int64_t)ots_partials(K) * LDW_N * 4 <= img_bytes, "the partial maxima do not fit the image region");
  CHECK(out_elems <= (int64_t)OTS_MAX_RANGES * LDW_N * n_all, "the slabs leave the 64 the workspace holds");

  const int cpr = n_all / 4;                                   // live 16-byte chunks per row of g
  std::vector<uint64_t> fetched((size_t)(((int64_t)K * cpr + 63) / 64), 0);
  std::vector<uint8_t> stored((size_t)out_elems, 0);
  int64_t clamped_cols = 0, repeats = 0, total_pieces = 0;
  CHECK((32 * (int64_t)cpr) % 64 == 0, "bitmap words straddle pieces");

  for (int by = 0; by < ranges; ++by) {
    const int k_begin = by * kps, np = ldw_range_pieces(K, kps, by);
    CHECK(np >= 1, "range %d is empty", by);
    total_pieces += np;
    // g: pieces 0 .. np + 2 are asked for (the prologue's four and s + 4 up to s = np - 1); threads take the pieces in turn
    // (a piece's 32 rows are whole 64-bit words of the bitmap)
    const int nthreads = (int)std::thread::hardware_concurrency() >= 8 ? 8 : 2;
    std::vector<int64_t> th_clamped(nthreads, 0), th_repeats(nthreads, 0);
    auto walk = [&](int th) {
      int64_t cl = 0, rp = 0;
      for (int piece = th; piece < np + 3; piece += nthreads)
        for (int bx = 0; bx < nbx; ++bx)
          for (int w = 0; w < 8; ++w)
            for (int i = 0; i < 2; ++i) {
              const int I = ots_g_dma_kib(i, w);
              for (int l = 0; l < 64; ++l) {
                const int t = ots_g_dma_row(I, l), c = ots_g_dma_chunk(I, l);
                const int colc = ots_g_col(bx, c, n_all);
                const bool real_col = bx * OTS_COLS + 4 * c < n_all;
                const int64_t off = ots_g_src(k_begin, piece, np, t, ldg, colc);
                const int64_t row = off / ldg;
                // the kernel forms the address as (piece 0's) + min(piece, np - 1) * 32 * ldg
                CHECK(off == ots_g_src(k_begin, 0, 1, t, ldg, colc) + (int64_t)ldw_min_i(piece, np - 1) * LDW_KP * ldg, "address split");
                CHECK(row >= k_begin && row < k_begin + (int64_t)np * LDW_KP && row < K && off - row * ldg == colc && colc >= 0 &&
                          colc + 4 <= n_all && (off & 3) == 0 && off + 4 <= g_floats && (!real_col || colc == bx * OTS_COLS + 4 * c),
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
    for (int th = 0; th < nthreads; ++th) { pool[th].join(); clamped_cols += th_clamped[th]; repeats += th_repeats[th]; }
    for (int bx = 0; bx < nbx; ++bx)
      for (int w = 0; w < 8; ++w) {
        const int c0 = bx * OTS_COLS + 16 * w;
        // X: pieces 0 .. np - 1 (and the clamped np - 1 once more) of the range, image k_begin / 32 + piece
        for (int e = 0; e < 5; ++e)
          for (int piece = 0; piece < np; piece += (np > 1 ? np - 1 : 1)) {      // first and last: the offset is linear in between
            const int64_t a = (int64_t)(k_begin / LDW_KP) * OTS_XPIECE + ots_x_dma_src(piece, ots_x_dma_kib(e, w), 63);
            CHECK(a >= 0 && a + 16 <= img_bytes, "image source %lld of %lld", (long long)a, (long long)img_bytes);
          }
        // the stores of an active wave: sixteen columns of ONE block
        if (c0 >= n_all) continue;
        CHECK(c0 / nb_cols == (c0 + 15) / nb_cols && c0 + 15 < n_all, "wave at column %d straddles two blocks", c0);
        for (int l = 0; l < 64; ++l) {
          const int r = l & 15, q = l >> 4, col = c0 + r;
          for (int j = 0; j < LDW_NT; ++j) {
            CHECK(4 * q + 16 * j + 3 < LDW_N, "exponent read");
            for (int i = 0; i < 4; ++i) {
              const int d = ldw_out_row(j, q, i);
              const int64_t o = ots_out_elem(by, slab, blk_stride, nb_cols, d, col);
              const int b = col / nb_cols;
              CHECK(d >= 0 && d < LDW_N && o >= 0 && o < out_elems, "store (%d, %d) at %lld", d, col, (long long)o);
              CHECK(o == ((int64_t)b * ranges + by) * slab + (int64_t)d * nb_cols + (col - b * nb_cols), "store (%d, %d) not in block %d", d, col, b);
              CHECK(!stored[o]++, "element %lld stored twice", (long long)o);
            }
          }
        }
      }
  }
  CHECK(total_pieces == npieces, "the ranges hold %lld pieces of %d", (long long)total_pieces, npieces);
  for (int64_t wd = 0; wd < ((int64_t)K * cpr + 63) / 64; ++wd) {
    const int64_t left = (int64_t)K * cpr - wd * 64;
    const uint64_t wantm = left >= 64 ? ~0ull : (1ull << left) - 1;
    CHECK(fetched[(size_t)wd] == wantm, "chunks %lld .. %lld: fetched mask %llx", (long long)(wd * 64), (long long)(wd * 64 + 63),
          (unsigned long long)fetched[(size_t)wd]);
  }
  for (size_t o = 0; o < stored.size(); ++o) CHECK(stored[o] == 1, "slab element %zu stored %d times", o, stored[o]);
  // the plane pass: block b writes image b from 32 rows of x
  for (int b = 0; b < npieces; b += (npieces > 1 ? npieces - 1 : 1)) {
    CHECK((int64_t)(b + 1) * OTS_XPIECE <= img_bytes, "image %d", b);
    for (int k = 0; k < LDW_KP; ++k) CHECK((int64_t)b * LDW_KP + k < K, "x row of image %d", b);
  }
  std::printf("K %d columns %d x %d (ldg %lld): %d K ranges of %d tokens (plan %d), %d column blocks; every g chunk fetched once, "
              "%lld clamped column fetches, %lld repeated fetches behind a range's end; every slab element stored once\n",
              K, nbatch, nb_cols, (long long)ldg, ranges, kps, pl, nbx, (long long)clamped_cols, (long long)repeats);
}

int main(int argc, char** argv) {
  check_layouts();
  std::printf("layouts: image, DMA, fragment and ring reads agree; transposed read free of bank conflicts\n");
  check_scale();
  std::printf("running exponent: below 2^15, only ever falls\n");
  CHECK(argc >= 5 && argc % 4 == 1, "usage: %s K nb_cols nbatch ldg [..]", argv[0]);
  for (int a = 1; a + 3 < argc; a += 4) check_shape(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]), std::atoll(argv[a + 3]));
  return 0;
}
