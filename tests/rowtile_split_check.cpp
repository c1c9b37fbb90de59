// Host checker of pydynet_amd/csrc/rowtile_split_index.h, the header from which the split-fp16 q | k | v and gate | up kernels
// (csrc/rowtile_split.hip) take every address they form.  Stand-alone (its own main), built by
// tests/test_rowtile_split_check_cpu.py under AddressSanitizer / UndefinedBehaviorSanitizer.
//
//   rowtile_split_check  kind M NF L hd up_first  [kind M NF L hd up_first ...]
//     kind 3: q | k | v, NF = D (three blocks of D columns), RoPE on the first 2 D columns with an (L x hd x 2) table
//     kind 1: gate | up, NF = F; up_first: the up matrix lies below the gate matrix in memory
//
// For every workgroup, wave, lane, tile and drain step it replays the index arithmetic against model buffers and checks:
// global elements inside their buffers, LDS offsets inside the allocation, the W image equal to what the fragment reads
// address (and free of bank conflicts), every weight read once, every element of qkv / gu / h / xn / rms written exactly
// once, every gate column beside its own up column and every RoPE pair on its own table entry -- across grid.y cuts too.
#include "../pydynet_amd/csrc/rowtile_split_index.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_fail = 0;
#define CHECK(cond, ...)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

struct Shape { int kind; int64_t M; int NF, L, hd, up_first; };

static void check_shape(const Shape& sh) {
  const int kind = sh.kind, K = RTS_K;
  const int64_t M = sh.M;
  const int F = kind == 1 ? sh.NF : 0, D = kind == 3 ? sh.NF : 0;
  const int N = kind == 1 ? 2 * F : 3 * D, nblocks = kind == 1 ? 2 : 3, nper = N / nblocks;
  const int ntiles = kind == 1 ? F / 16 : N / 32;
  const int64_t ldb = nper, bstride = (int64_t)K * nper + 64;              // blocks a little further apart than they are large
  const unsigned g_off = kind == 1 && sh.up_first ? (unsigned)bstride : 0u, u_off = kind == 1 && !sh.up_first ? (unsigned)bstride : 0u;
  const int64_t wfloats = bstride * (nblocks - 1) + (int64_t)K * nper;
  const int64_t ldc = N, ldh = F, lda = K, ldxn = K;
  CHECK(RTS_LDS <= 160 * 1024, "LDS %d", RTS_LDS);

  // ---- W pass: every weight read once, every unit of the image written once; what the fragments then address -----------
  {
    std::vector<unsigned char> wseen((size_t)wfloats, 0);
    for (int tile = 0; tile < ntiles; ++tile) {
      std::vector<int> unit_n(RTS_PLANE / 16, -1), unit_u(RTS_PLANE / 16, -1);
      for (int tid = 0; tid < 256; ++tid) {
        const int c = tid & 31, kq = tid >> 5;
        for (int k = kq; k < K; k += 8) {
          const int64_t o = rts_w_src(kind, tile, c, k, nper, ldb, bstride, g_off, u_off);
          CHECK(o >= 0 && o < wfloats, "W source %lld of %lld", (long long)o, (long long)wfloats);
          if (o >= 0 && o < wfloats) { CHECK(!wseen[(size_t)o], "W element read twice"); wseen[(size_t)o] = 1; }
          // the column a tile column stands for
          const int col = kind == 1 ? 16 * tile + (c & 15) : (32 * tile + c) % nper;
          const int64_t base = kind == 1 ? (c < 16 ? g_off : u_off) : (int64_t)((32 * tile + c) / nper) * bstride;
          CHECK(o == base + (int64_t)k * ldb + col, "W source of tile %d column %d", tile, c);
        }
        for (int u = tid; u < 32 * 36; u += 256) {
          const int ku = u >> 5;
          CHECK((u & 31) == c, "unit column");
          const int off = rts_img_unit(c, ku);
          CHECK(off >= 0 && off + 16 <= RTS_PLANE && off % 16 == 0, "image unit offset %d", off);
          if (off >= 0 && off + 16 <= RTS_PLANE) {
            CHECK(unit_n[off / 16] < 0, "image unit written twice");
            unit_n[off / 16] = c; unit_u[off / 16] = ku;
          }
        }
      }
      for (size_t i = 0; i < unit_n.size(); ++i) CHECK(unit_n[i] >= 0, "image unit %zu never written", i);
      if (tile == 0)
        for (int s = 0; s < RTS_KS; ++s)
          for (int lh = 0; lh < 2; ++lh) {
            int slots[2] = {0, 0};
            for (int li = 0; li < 32; ++li) {
              const int off = rts_frag_base(li, lh, s & 1) + rts_frag_step(s);
              CHECK(off >= 0 && off + 16 <= RTS_PLANE, "fragment offset %d", off);
              CHECK(unit_n[off / 16] == li && unit_u[off / 16] == 2 * s + lh, "fragment of lane (%d, %d), k-step %d reads column %d unit %d",
                    li, lh, s, unit_n[off / 16], unit_u[off / 16]);
              CHECK(8 * unit_u[off / 16] == rts_a_col(s, lh), "W and x fragments on different k");
              slots[li >> 4] |= 1 << ((off / 16) & 15);              // sixteen lanes of a ds_read_b128: sixteen different slots
            }
            CHECK(slots[0] == 0xffff && slots[1] == 0xffff, "bank conflict in k-step %d", s);
          }
    }
    int64_t nread = 0;
    for (size_t i = 0; i < wseen.size(); ++i) nread += wseen[i];
    CHECK(nread == (int64_t)K * N, "%lld weights read, %lld exist", (long long)nread, (long long)K * N);
  }
  // ---- staging of an image ----------------------------------------------------------------------------------------
  {
    std::vector<int> seen(RTS_UNITS, 0);
    for (int q = 0; q < 5; ++q)
      for (int tid = 0; tid < 512; ++tid)
        if (q < 4 || rts_stage_on(q, tid)) {
          const int u = rts_stage_unit(q, tid);
          CHECK(u >= 0 && u < RTS_UNITS, "staged unit %d", u);
          if (u >= 0 && u < RTS_UNITS) ++seen[u];
          CHECK(2 * RTS_TILE + u * 16 + 16 <= 3 * RTS_TILE, "staged unit past the ring");
        }
    for (int u = 0; u < RTS_UNITS; ++u) CHECK(seen[u] == 1, "unit %d staged %d times", u, seen[u]);
    CHECK(RTS_TAIL + 128 + 32 * 4 == RTS_TILE, "tail");
  }
  // ---- the staging area of a wave: what a store reads is what the drain wrote ------------------------------------------
  {
    std::vector<int> row(RTS_STG / 16, -1), col(RTS_STG / 16, -1);
    for (int lane = 0; lane < 64; ++lane)
      for (int g = 0; g < 4; ++g) {
        const int li = lane & 31, lh = lane >> 5, off = rts_stg_w(li, lh, g);
        CHECK(off >= 0 && off + 16 <= RTS_STG && off % 16 == 0, "staging write %d", off);
        CHECK(row[off / 16] < 0, "staging unit written twice");
        row[off / 16] = li; col[off / 16] = rts_reg_col(g, lh);
        // the exponents of these four columns: tail + 4 * column
        CHECK(RTS_TAIL + 4 * rts_reg_col(0, lh) + 32 * g == RTS_TAIL + 4 * rts_reg_col(g, lh), "exponent address");
      }
    std::vector<int> cover(32 * 8, 0);
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 4; ++j) {
        const int off = rts_stg_r(lane, j);
        CHECK(off >= 0 && off + 16 <= RTS_STG, "staging read %d", off);
        CHECK(row[off / 16] == rts_st_row(lane, j) && col[off / 16] == rts_st_col(lane), "store %d of lane %d reads row %d column %d", j,
              lane, row[off / 16], col[off / 16]);
        ++cover[rts_st_row(lane, j) * 8 + rts_st_col(lane) / 4];
      }
    for (int i = 0; i < 32 * 8; ++i) CHECK(cover[i] == 1, "tile unit %d stored %d times", i, cover[i]);
    if (kind == 1) {
      std::vector<int> hrow(RTS_STG / 16, -1), hcol(RTS_STG / 16, -1);
      for (int lane = 0; lane < 64; ++lane)
        for (int g = 0; g < 2; ++g) {
          const int li = lane & 31, lh = lane >> 5, off = rts_h_w(li, lh, g);
          CHECK(off >= 0 && off + 16 <= RTS_STG, "h write %d", off);
          CHECK(hrow[off / 16] < 0, "h unit written twice");
          hrow[off / 16] = li; hcol[off / 16] = rts_reg_col(g, lh);
          for (int i = 0; i < 4; ++i) {
            // gate in register 4 g + i, up in register 4 g + 8 + i of the same lane: the same column of their matrices
            const int cg = rts_reg_col(g, lh) + i, cu = rts_reg_col(g + 2, lh) + i;
            CHECK(cg < 16 && cu == cg + 16, "gate / up registers of group %d", g);
            for (int t = 0; t < ntiles; ++t) {
              const int og = rts_out_col(1, t, cg, F), ou = rts_out_col(1, t, cu, F);
              CHECK(og < F && ou == og + F, "gate column %d beside up column %d", og, ou - F);
              CHECK(rts_w_src(1, t, cg, 0, nper, ldb, bstride, g_off, u_off) == (int64_t)g_off + og, "gate weights");
              CHECK(rts_w_src(1, t, cu, 0, nper, ldb, bstride, g_off, u_off) == (int64_t)u_off + og, "up weights");
            }
          }
        }
      std::vector<int> hc(32 * 4, 0);
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 2; ++j) {
          const int off = rts_h_r(lane, j);
          CHECK(off >= 0 && off + 16 <= RTS_STG, "h read %d", off);
          CHECK(hrow[off / 16] == rts_h_row(lane, j) && hcol[off / 16] == 4 * (lane & 3), "h store %d of lane %d", j, lane);
          CHECK(rts_h_col(3, lane) == rts_out_col(1, 3, 4 * (lane & 3), F), "h column");
          ++hc[rts_h_row(lane, j) * 4 + (lane & 3)];
        }
      for (int i = 0; i < 32 * 4; ++i) CHECK(hc[i] == 1, "h unit %d stored %d times", i, hc[i]);
    }
  }
  // ---- RoPE: pairs inside a lane's four columns and one head, on the table entry of the lane's row ------------------------
  if (kind == 3) {
    const unsigned magic = rts_rope_magic(sh.hd);
    for (unsigned c = 0; c < 65536; ++c) CHECK(rts_rope_colh_magic(c, (unsigned)sh.hd, magic) == c % (unsigned)sh.hd, "magic division of %u", c);
    const int rope_tiles = 2 * D / 32;
    CHECK(sh.hd % 4 == 0 && D % sh.hd == 0 && M % sh.L == 0, "shape");
    for (int t = 0; t < rope_tiles; ++t)
      for (int g = 0; g < 4; ++g)
        for (int lh = 0; lh < 2; ++lh) {
          const int c = 32 * t + rts_reg_col(g, lh), colh = rts_rope_colh(t, g, lh, sh.hd);
          CHECK(c % 2 == 0 && colh == (c % D) % sh.hd && colh + 3 < sh.hd, "pair of column %d", c);
          CHECK((int)rts_rope_colh_magic((unsigned)c, (unsigned)sh.hd, magic) == colh, "column in head");
          CHECK(rts_out_col(3, t, rts_reg_col(g, lh), 0) == c, "output column");
        }
  }
  // ---- the grid: rows, column ranges, every output element once ------------------------------------------------------------
  int tpw, parts;
  rts_plan(M, ntiles, &tpw, &parts);
  const int64_t row_blocks = (M + 255) / 256;
  CHECK(parts >= 1 && (row_blocks * parts >= 256 || parts == ntiles), "plan: %d parts", parts);
  std::vector<int> tile_owner(ntiles, 0);
  for (int y = 0; y < parts; ++y) {
    const int T0 = y * tpw, T1 = rts_min_i(ntiles, T0 + tpw);
    CHECK(T0 < T1, "empty column range %d", y);
    for (int t = T0; t < T1; ++t) ++tile_owner[t];
  }
  for (int t = 0; t < ntiles; ++t) CHECK(tile_owner[t] == 1, "tile %d in %d ranges", t, tile_owner[t]);
  std::vector<unsigned char> c_cnt((size_t)(M * ldc / 4), 0), h_cnt((size_t)(kind == 1 ? M * ldh / 4 : 0), 0);
  std::vector<unsigned char> xn_cnt((size_t)(M * ldxn / 4), 0), rms_cnt((size_t)M, 0);
  for (int64_t bx = 0; bx < row_blocks; ++bx)
    for (int y = 0; y < parts; ++y) {
      const int T0 = y * tpw, T1 = rts_min_i(ntiles, T0 + tpw);
      for (int wave = 0; wave < 8; ++wave) {
        const int64_t m0 = (bx * 8 + wave) * 32;
        for (int lane = 0; lane < 64; ++lane) {
          const int li = lane & 31, lh = lane >> 5;
          const int64_t r = rts_a_row(m0, li, M);
          CHECK(r >= 0 && r < M, "A row");
          for (int s = 0; s < RTS_KS; ++s) {
            const int64_t e = r * lda + rts_a_col(s, lh);
            CHECK(rts_a_col(s, lh) + 8 <= K && e + 8 <= M * lda, "A element");
            if (y == 0 && m0 + li < M) { ++xn_cnt[(size_t)((r * ldxn + rts_a_col(s, lh)) / 4)]; ++xn_cnt[(size_t)((r * ldxn + rts_a_col(s, lh)) / 4 + 1)]; }
          }
          if (y == 0 && lh == 0 && m0 + li < M) ++rms_cnt[(size_t)(m0 + li)];
          if (kind == 3) {
            const int pos = rts_rope_pos(m0, li, sh.L);
            CHECK(m0 + li >= M || pos == (int)((m0 + li) % sh.L), "position");
            for (int t = T0; t < T1 && t < 2 * D / 32; ++t)
              for (int g = 0; g < 4; ++g) {
                const int e = rts_rope_entry(pos, rts_rope_colh(t, g, lh, sh.hd), sh.hd);
                CHECK(e >= 0 && e + 8 <= sh.L * sh.hd * 2, "table entry %d", e);
              }
          }
          for (int t = T0; t < T1; ++t) {
            for (int j = 0; j < 4; ++j) {
              const int64_t row = m0 + rts_st_row(lane, j);
              if (row >= M) continue;
              const int col = rts_out_col(kind, t, rts_st_col(lane), F);
              CHECK(col % 4 == 0 && col + 4 <= N && rts_out_col(kind, t, rts_st_col(lane) + 3, F) == col + 3, "output column %d", col);
              ++c_cnt[(size_t)((row * ldc + col) / 4)];
            }
            if (kind == 1)
              for (int j = 0; j < 2; ++j) {
                const int64_t row = m0 + rts_h_row(lane, j);
                if (row >= M) continue;
                const int col = rts_h_col(t, lane);
                CHECK(col % 4 == 0 && col + 4 <= F, "h column %d", col);
                ++h_cnt[(size_t)((row * ldh + col) / 4)];
              }
          }
        }
      }
    }
  int64_t bad = 0;
  for (size_t i = 0; i < c_cnt.size(); ++i) bad += c_cnt[i] != 1;
  for (size_t i = 0; i < h_cnt.size(); ++i) bad += h_cnt[i] != 1;
  for (size_t i = 0; i < xn_cnt.size(); ++i) bad += xn_cnt[i] != 1;
  for (size_t i = 0; i < rms_cnt.size(); ++i) bad += rms_cnt[i] != 1;
  CHECK(bad == 0, "%lld output units not written exactly once", (long long)bad);
  if (!g_fail)
    printf("kind %d M %lld N %d (L %d hd %d up_first %d): %d tiles in %d ranges, every output element written once\n", kind, (long long)M, N,
           sh.L, sh.hd, sh.up_first, ntiles, parts);
}

int main(int argc, char** argv) {
  if (argc < 7 || (argc - 1) % 6 != 0) { printf("usage: %s kind M NF L hd up_first ...\n", argv[0]); return 2; }
  for (int i = 1; i + 5 < argc; i += 6) {
    Shape s{atoi(argv[i]), atoll(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]), atoi(argv[i + 5])};
    check_shape(s);
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  }
  return 0;
}
