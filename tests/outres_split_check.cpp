// Host checker of pydynet_amd/csrc/outres_split_index.h, the header from which the split-fp16 output-resident products
// (csrc/outres_split.hip) take every address they form.  Stand-alone (its own main), built by
// tests/test_outres_split_check_cpu.py under AddressSanitizer / UndefinedBehaviorSanitizer.
//
//   outres_split_check  form M K nb neg lda_pad ldc_pad  [form M K nb neg lda_pad ldc_pad ...]
//     form 0: NT, B = nb blocks (288 x K / nb); neg: the blocks lie at falling addresses;  form 1: NN, B (K x 288)
//
// It replays the W pass and the persistent main kernel -- every workgroup, block, wave, lane, piece and store step, in the
// kernel's order -- against model buffers and checks: global elements inside their buffers, LDS offsets inside the
// allocation, every weight read once, the image equal to what the fragments address and free of bank conflicts, every A
// chunk fetched exactly once and found in the ring where its lane reads it, the W slot and the ring slot of every piece
// holding that piece when it is used, every row block visited exactly once, every element of C written exactly once, rows
// past M never read or written.
#include "../pydynet_amd/csrc/outres_split_index.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

struct Shape { int form; int64_t M; int K, nb, neg, lda_pad, ldc_pad; };

static void check_shape(const Shape& sh) {
  const int64_t M = sh.M;
  const int K = sh.K, np = K / ORS_KP, nn = sh.form == 1, nb = nn ? 1 : sh.nb, kb = K / nb, ppb = kb / ORS_KP;
  const int64_t lda = K + sh.lda_pad, ldc = ORS_N + sh.ldc_pad;
  CHECK(ORS_LDS <= 160 * 1024, "LDS %d", ORS_LDS);
  CHECK(K % ORS_KP == 0 && K >= ORS_MIN_K && K <= ORS_MAX_K && kb * nb == K && kb % ORS_KP == 0 && np >= 2 * ORS_RING, "shape");

  // ---- W pass: every weight read once, every unit of an image written once; what the fragments then address -------------
  {
    const int64_t ldb = nn ? ORS_N + 32 : kb, blk_floats = (int64_t)ORS_N * ldb;
    const int64_t bstride = (blk_floats + 64) * (sh.neg ? -1 : 1);
    const int64_t wfloats = nn ? (int64_t)(K - 1) * ldb + ORS_N : (blk_floats + 64) * (nb - 1) + blk_floats;
    const int64_t base = sh.neg ? (blk_floats + 64) * (nb - 1) : 0;          // where block 0 lies in the buffer
    std::vector<unsigned char> wseen((size_t)wfloats, 0);
    for (int piece = 0; piece < np; ++piece) {
      std::vector<int> unit_d(ORS_PLANE / 16, -1), unit_q(ORS_PLANE / 16, -1);
      std::vector<int> tile(ORS_KP * ORS_NN_LD, -1);                         // NN: which (k, d) an LDS float holds
      if (nn)
        for (int i = 0; i < ORS_KP * (ORS_N / 4); ++i) {
          const int64_t o = ors_w_src_nn(piece, i, ldb);
          CHECK(o >= 0 && o + 4 <= wfloats, "B source %lld of %lld", (long long)o, (long long)wfloats);
          for (int c = 0; c < 4; ++c) {
            const int l = ors_nn_lds(i / 72, 4 * (i % 72) + c);
            CHECK(l >= 0 && l < ORS_KP * ORS_NN_LD && tile[l] < 0, "LDS tile float %d", l);
            if (l >= 0 && l < ORS_KP * ORS_NN_LD) tile[l] = (i / 72) * ORS_N + 4 * (i % 72) + c;
            if (o >= 0 && o + 4 <= wfloats) { CHECK(!wseen[(size_t)(o + c)], "B element read twice"); wseen[(size_t)(o + c)] = 1; }
            CHECK(o + c == ((int64_t)piece * ORS_KP + i / 72) * ldb + 4 * (i % 72) + c, "B element");
          }
        }
      for (int i = 0; i < ORS_N * 4; ++i) {
        const int d = i >> 2, q = i & 3;
        if (nn) {
          for (int j = 0; j < 8; ++j) {
            const int l = ors_nn_lds(8 * q + j, d);
            CHECK(l >= 0 && l < ORS_KP * ORS_NN_LD && tile[l] == (8 * q + j) * ORS_N + d, "transposed read of (%d, %d)", 8 * q + j, d);
          }
        } else {
          const int64_t o = base + ors_w_src_nt(piece, d, q, ppb, ldb, bstride);
          CHECK(o >= 0 && o + 8 <= wfloats, "W source %lld of %lld", (long long)o, (long long)wfloats);
          const int b = piece / ppb;
          CHECK(o == base + b * bstride + (int64_t)d * ldb + (piece % ppb) * ORS_KP + 8 * q, "W source of piece %d column %d", piece, d);
          if (o >= 0 && o + 8 <= wfloats)
            for (int c = 0; c < 8; ++c) { CHECK(!wseen[(size_t)(o + c)], "W element read twice"); wseen[(size_t)(o + c)] = 1; }
        }
        const int off = ors_img_unit(d, q);
        CHECK(off >= 0 && off + 16 <= ORS_PLANE && off % 16 == 0, "image unit offset %d", off);
        if (off >= 0 && off + 16 <= ORS_PLANE) {
          CHECK(unit_d[off / 16] < 0, "image unit written twice");
          unit_d[off / 16] = d; unit_q[off / 16] = q;
        }
      }
      for (size_t i = 0; i < unit_d.size(); ++i) CHECK(unit_d[i] >= 0, "image unit %zu never written", i);
      if (piece == 0)
        for (int j = 0; j < ORS_NT; ++j) {
          int cover[16] = {0};
          for (int g16 = 0; g16 < 4; ++g16) {
            int slots = 0;
            for (int l = 0; l < 16; ++l) {
              const int lane = 16 * g16 + l, r = lane & 15, q = lane >> 4, off = ors_frag(r, q) + 1024 * j;
              CHECK(off >= 0 && off + 16 <= ORS_PLANE, "fragment offset %d", off);
              CHECK(unit_d[off / 16] == 16 * j + r && unit_q[off / 16] == q, "fragment of lane (%d, %d), tile %d reads column %d unit %d", r, q,
                    j, unit_d[off / 16], unit_q[off / 16]);
              slots |= 1 << ((off / 16) & 15);
              ++cover[(off / 16) & 15];
            }
            CHECK(slots == 0xffff, "bank conflict in tile %d", j);       // sixteen lanes served together: sixteen slots
          }
          for (int i = 0; i < 16; ++i) CHECK(cover[i] == 4, "slot %d read %d times", i, cover[i]);
        }
    }
    int64_t nread = 0;
    for (size_t i = 0; i < wseen.size(); ++i) nread += wseen[i];
    CHECK(nread == (int64_t)K * ORS_N, "%lld weights read, %lld exist", (long long)nread, (long long)K * ORS_N);
    // the DMA of an image: 36 instructions of 1 KiB, every one issued by some wave, inside the slot
    int seen[36] = {0};
    for (int wave = 0; wave < 8; ++wave)
      for (int e = 0; e < 5; ++e) {
        const int I = ors_wdma_instr(e, wave);
        CHECK(I >= 0 && I < 36 && I * 1024 + 63 * 16 + 16 <= ORS_PIECE, "W DMA instruction %d", I);
        if (I >= 0 && I < 36) ++seen[I];
      }
    for (int I = 0; I < 36; ++I) CHECK(seen[I] >= 1, "W DMA instruction %d never issued", I);
  }

  // ---- the ring of a wave: what a lane reads is what the DMA put there, conflict free ---------------------------------------
  {
    std::vector<int> row(ORS_RAW / 16, -1), chunk(ORS_RAW / 16, -1);
    for (int i = 0; i < 2; ++i)
      for (int lane = 0; lane < 64; ++lane) {
        const int off = 1024 * i + 16 * lane;
        CHECK(row[off / 16] < 0, "ring unit written twice");
        row[off / 16] = ors_raw_row(i, lane); chunk[off / 16] = ors_raw_chunk(i, lane);
        CHECK(chunk[off / 16] >= 0 && chunk[off / 16] < 8 && row[off / 16] < 16, "ring unit");
      }
    for (int half = 0; half < 2; ++half)
      for (int g16 = 0; g16 < 4; ++g16) {
        int slots = 0;
        for (int l = 0; l < 16; ++l) {
          const int lane = 16 * g16 + l, r = lane & 15, q = lane >> 4, off = ors_raw_lane(r, q) ^ (16 * half);
          CHECK(off >= 0 && off + 16 <= ORS_RAW, "ring read %d", off);
          CHECK(row[off / 16] == r && chunk[off / 16] == 2 * q + half, "lane (%d, %d) reads row %d chunk %d", r, q, row[off / 16], chunk[off / 16]);
          slots |= 1 << ((off / 16) & 15);
        }
        CHECK(slots == 0xffff, "bank conflict in the ring read");
      }
  }

  // ---- the persistent walk -----------------------------------------------------------------------------------------------------
  const int nblk = ors_blocks(M), grid = ors_grid(M);
  const int64_t afloats = (M - 1) * lda + K, cfloats = (M - 1) * ldc + ORS_N;
  std::vector<unsigned char> a_cnt((size_t)(M * (K / 4)), 0), c_cnt((size_t)(M * (ORS_N / 4)), 0), visited((size_t)nblk, 0);
  CHECK(grid >= 1 && grid <= ORS_MAX_WGS && grid <= nblk, "grid %d", grid);
  auto fetch = [&](int blk, int wave, int piece, int ring, bool count) {            // the two DMA instructions of a piece of A
    CHECK(piece >= 0 && piece < np && ring >= 0 && ring < ORS_RING, "piece %d ring %d", piece, ring);
    for (int i = 0; i < 2; ++i)
      for (int lane = 0; lane < 64; ++lane) {
        const int rr = ors_raw_row(i, lane), ch = ors_raw_chunk(i, lane);
        const int64_t arow = ors_a_row(blk, wave, rr, M), o = arow * lda + (int64_t)piece * ORS_KP + 4 * ch;
        CHECK(arow >= 0 && arow < M && o >= 0 && o + 4 <= afloats, "A element %lld of %lld", (long long)o, (long long)afloats);
        const int dst = ORS_RING0 + wave * (ORS_RING * ORS_RAW) + ring * ORS_RAW + 1024 * i + 16 * lane;
        CHECK(dst >= ORS_RING0 && dst + 16 <= ORS_LDS, "ring destination %d", dst);
        if (count && (int64_t)blk * ORS_WG_ROWS + wave * 16 + rr < M && arow >= 0 && arow < M)      // (clamped rows: repeats of row M - 1)
          ++a_cnt[(size_t)(arow * (K / 4) + piece * 8 + ch)];
      }
  };
  for (int x = 0; x < grid; ++x)
    for (int wave = 0; wave < 8; ++wave) {
      struct Tag { int blk, piece; };
      Tag ring[ORS_RING], wslot[2] = {{-1, 0}, {-1, -1}};                // W slots: the piece they hold (blk unused)
      int blk = x, nxt = ors_next_block(blk, grid, nblk), cur = 0, g = 0;
      wslot[0].piece = 0;
      for (int i = 0; i < ORS_RING; ++i) { fetch(blk, wave, i, i, true); ring[i] = {blk, i}; }
      Tag planes = ring[0];                                              // the piece whose planes are in registers
      for (;;) {
        CHECK(blk >= 0 && blk < nblk, "block %d", blk);
        if (wave == 0 && blk >= 0 && blk < nblk) ++visited[(size_t)blk];
        for (int s = 0; s < np; ++s, ++g) {
          const bool last = s + 1 == np;
          CHECK(wslot[cur].piece == s, "W slot holds piece %d at piece %d", wslot[cur].piece, s);
          CHECK(planes.blk == blk && planes.piece == s, "planes of block %d piece %d at block %d piece %d", planes.blk, planes.piece, blk, s);
          wslot[1 - cur].piece = last ? 0 : s + 1;
          const int rs = g & (ORS_RING - 1);
          CHECK(ring[rs].blk == blk && ring[rs].piece == s, "ring slot overwritten before its piece ran");
          const int ab = ors_ahead_next(s, np) ? nxt : blk, ap = ors_ahead_piece(s, np);
          CHECK(ors_ahead_next(s, np) == (s + ORS_RING >= np) && ap == (s + ORS_RING) % np, "piece ahead");
          const bool repeat = ab == blk && ors_ahead_next(s, np);       // behind the last block: the block's first pieces again
          if (repeat) CHECK(nxt == blk && ap < ORS_RING, "repeated fetch");
          fetch(ab, wave, ap, rs, !repeat);
          ring[rs] = {ab, ap};
          const Tag nx = ring[(g + 1) & (ORS_RING - 1)];
          if (!last) CHECK(nx.blk == blk && nx.piece == s + 1, "next piece in the ring: block %d piece %d", nx.blk, nx.piece);
          else CHECK(nx.blk == nxt && nx.piece == 0, "first piece of the next block in the ring: block %d piece %d", nx.blk, nx.piece);
          planes = nx;
          cur = 1 - cur;
        }
        for (int lane = 0; lane < 64; ++lane) {
          const int r = lane & 15, q = lane >> 4;
          const int64_t row = (int64_t)blk * ORS_WG_ROWS + wave * 16 + r;
          if (row >= M) continue;
          for (int j = 0; j < ORS_NT; ++j) {
            const int col = ors_out_col(j, q);
            const int64_t o = row * ldc + col;
            CHECK(col % 4 == 0 && col + 4 <= ORS_N && o >= 0 && o + 4 <= cfloats, "C element %lld of %lld", (long long)o, (long long)cfloats);
            ++c_cnt[(size_t)(row * (ORS_N / 4) + col / 4)];
          }
        }
        if (nxt == blk) break;
        blk = nxt;
        nxt = ors_next_block(blk, grid, nblk);
      }
    }
  int64_t bad = 0;
  for (size_t i = 0; i < a_cnt.size(); ++i) bad += a_cnt[i] != 1;
  CHECK(bad == 0, "%lld chunks of A not fetched exactly once", (long long)bad);
  bad = 0;
  for (size_t i = 0; i < c_cnt.size(); ++i) bad += c_cnt[i] != 1;
  CHECK(bad == 0, "%lld units of C not written exactly once", (long long)bad);
  bad = 0;
  for (size_t i = 0; i < visited.size(); ++i) bad += visited[i] != 1;
  CHECK(bad == 0, "%lld row blocks not visited exactly once", (long long)bad);
  // the exponent rule: S only falls, a maximum below 2^15 at the old scale moves nothing, a set maximum lands in [2^12, 2^13)
  for (int E = -148; E <= 128; ++E) {
    const int S0 = ors_next_exp(true, E, ORS_UNSET);
    CHECK(S0 == 13 - E && ors_next_exp(false, E, ORS_UNSET) == ORS_UNSET, "first exponent");
    for (int dE = -40; dE <= 40; ++dE) {
      const int S1 = ors_next_exp(true, E + dE, S0);
      CHECK(S1 <= S0 && E + dE + S1 <= 15 && (dE <= 2 ? S1 == S0 : S1 == 13 - E - dE), "exponent step %d", dE);
    }
  }
  if (!g_fail)
    printf("form %d M %lld K %d (%d blocks, neg %d, lda %lld, ldc %lld): %d row blocks on %d workgroups, every chunk of A fetched once, "
           "every output element written once\n", sh.form, (long long)M, K, nb, sh.neg, (long long)lda, (long long)ldc, nblk, grid);
}

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 1) % 7 != 0) { printf("usage: %s form M K nb neg lda_pad ldc_pad ...\n", argv[0]); return 2; }
  for (int i = 1; i + 6 < argc; i += 7) {
    Shape s{atoi(argv[i]), atoll(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]), atoi(argv[i + 5]), atoi(argv[i + 6])};
    check_shape(s);
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  }
  return 0;
}
