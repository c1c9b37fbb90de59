// Host checker of the dh + SwiGLU backward form (rts_main_kernel<2>, kind 2 of rts_w_kernel) of csrc/rowtile_split.hip, through
// pydynet_amd/csrc/rowtile_split_index.h, the header from which the kernels take every address they form.  Stand-alone (its own
// main), built by tests/test_rowtile_split_bwd_check_cpu.py under AddressSanitizer / UndefinedBehaviorSanitizer.
//
//   rowtile_split_bwd_check  [b M F | p kind M NF] ...
//     b: the dh + SwiGLU backward form; p: the A prologue by whole 128-byte lines of form `kind` (1 gate | up, NF = F;
//     2 dh + SwiGLU backward, NF = F; 3 q | k | v, NF = D)
//
// dgu (M x 2F) = SwiGLU'(gu) o (g2 (M x 288) Wd^T), Wd (F x 288) row-major, gu / dgu packed [gate | up].  A tile is 32 dh
// columns = 32 rows of Wd.  For every workgroup, wave, lane, tile and store step it replays the index arithmetic against model
// buffers and checks: every weight read once by the W pass and inside Wd; the image where the fragments address it; every gu
// element read exactly once, by the lane that writes the matching dgu element; every dgu element written once and none behind
// row M or column 2F; each eight-lane group of a load or store on one aligned 128-byte line; LDS offsets inside RTS_LDS; the
// grid.y cuts covering every tile once.  For the prologue: every A element of a wave's 32 rows read once, every load
// instruction on eight whole lines, the staging round trip putting element (row, k) where the fragment read expects it,
// at most two lanes per LDS bank, xn and rms written exactly once, by the first column range only.
#include "../pydynet_amd/csrc/rowtile_split_index.h"
#include <cstdio>
#include <cstdlib>
#include <algorithm>
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

static void check_shape(int64_t M, int F) {
  const int K = RTS_K, ntiles = F / 32;
  const int64_t ldb = K + 4, ldc = 2 * (int64_t)F, lda = K;   // Wd rows a little further apart than they are long
  const int64_t wfloats = (int64_t)(F - 1) * ldb + K;
  CHECK(F % 32 == 0 && F >= 32, "F %d", F);
  CHECK(RTS_LDS <= 160 * 1024, "LDS %d", RTS_LDS);
  CHECK(ldc % 32 == 0, "a row of gu / dgu is a whole number of 128-byte lines");

  // ---- W pass, transposed source: every weight once; the image as in the other forms ------------------------------------
  {
    std::vector<unsigned char> wseen((size_t)wfloats, 0);
    for (int tile = 0; tile < ntiles; ++tile) {
      std::vector<int> smn(RTS_K * 33, -1), smk(RTS_K * 33, -1);       // the kernel's sm[k * 33 + n]
      for (int tid = 0; tid < 256; ++tid)
        for (int i = tid; i < 32 * K; i += 256) {
          const int n = rts_w_t_n(i), k = rts_w_t_k(i);
          CHECK(n >= 0 && n < 32 && k >= 0 && k < K && n * K + k == i, "element %d -> (%d, %d)", i, n, k);
          const int64_t o = rts_w_src_t(tile, n, k, ldb);
          CHECK(o >= 0 && o < wfloats, "W source %lld of %lld", (long long)o, (long long)wfloats);
          CHECK(o == (int64_t)rts_bwd_gate_col(tile, n) * ldb + k, "tile column %d is not row %d of Wd", n, rts_bwd_gate_col(tile, n));
          if (o >= 0 && o < wfloats) { CHECK(!wseen[(size_t)o], "W element read twice"); wseen[(size_t)o] = 1; }
          CHECK(smn[k * 33 + n] < 0, "sm written twice");
          smn[k * 33 + n] = n; smk[k * 33 + n] = k;
        }
      // the split phase reads sm[(8 ku + j) * 33 + c] for unit ku of column c and writes rts_img_unit(c, ku)
      std::vector<int> unit_n(RTS_PLANE / 16, -1), unit_u(RTS_PLANE / 16, -1);
      for (int tid = 0; tid < 256; ++tid) {
        const int c = tid & 31;
        for (int u = tid; u < 32 * 36; u += 256) {
          const int ku = u >> 5;
          CHECK((u & 31) == c, "unit column");
          for (int j = 0; j < 8; ++j) CHECK(smn[(8 * ku + j) * 33 + c] == c && smk[(8 * ku + j) * 33 + c] == 8 * ku + j, "sm element");
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
              CHECK(unit_n[off / 16] == li && unit_u[off / 16] == 2 * s + lh, "fragment of lane (%d, %d), k-step %d", li, lh, s);
              CHECK(8 * unit_u[off / 16] == rts_a_col(s, lh), "W and A fragments on different k");
              CHECK(2 * RTS_TILE + RTS_PLANE + off + 16 <= 3 * RTS_TILE, "fragment past the ring");
              slots[li >> 4] |= 1 << ((off / 16) & 15);
            }
            CHECK(slots[0] == 0xffff && slots[1] == 0xffff, "bank conflict in k-step %d", s);
          }
    }
    int64_t nread = 0;
    for (size_t i = 0; i < wseen.size(); ++i) nread += wseen[i];
    CHECK(nread == (int64_t)K * F, "%lld weights read, %lld exist", (long long)nread, (long long)K * F);
  }
  // ---- staging of an image, and the staging area of a wave ------------------------------------------------------------
  {
    std::vector<int> seen(RTS_UNITS, 0);
    for (int q = 0; q < 5; ++q)
      for (int tid = 0; tid < 512; ++tid)
        if (q < 4 || rts_stage_on(q, tid)) {
          const int u = rts_stage_unit(q, tid);
          CHECK(u >= 0 && u < RTS_UNITS, "staged unit %d", u);
          if (u >= 0 && u < RTS_UNITS) ++seen[u];
        }
    for (int u = 0; u < RTS_UNITS; ++u) CHECK(seen[u] == 1, "unit %d staged %d times", u, seen[u]);
    std::vector<int> row(RTS_STG / 16, -1), col(RTS_STG / 16, -1);
    for (int lane = 0; lane < 64; ++lane)
      for (int g = 0; g < 4; ++g) {
        const int li = lane & 31, lh = lane >> 5, off = rts_stg_w(li, lh, g);
        CHECK(off >= 0 && off + 16 <= RTS_STG && off % 16 == 0, "staging write %d", off);
        CHECK(3 * RTS_TILE + 7 * RTS_STG + off + 16 <= RTS_LDS, "staging area past the allocation");
        CHECK(row[off / 16] < 0, "staging unit written twice");
        row[off / 16] = li; col[off / 16] = rts_reg_col(g, lh);
        CHECK(RTS_TAIL + 4 * rts_reg_col(0, lh) + 32 * g + 16 <= RTS_TILE, "exponent address");
      }
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 4; ++j) {
        const int off = rts_stg_r(lane, j);
        CHECK(off >= 0 && off + 16 <= RTS_STG, "staging read %d", off);
        CHECK(row[off / 16] == rts_st_row(lane, j) && col[off / 16] == rts_st_col(lane), "store %d of lane %d reads row %d column %d", j,
              lane, row[off / 16], col[off / 16]);
      }
  }
  // ---- the grid ---------------------------------------------------------------------------------------------------------
  int tpw, parts;
  rts_plan(M, ntiles, &tpw, &parts);
  const int64_t row_blocks = (M + 255) / 256;
  CHECK(parts >= 1 && parts <= ntiles && tpw * parts >= ntiles && tpw * (parts - 1) < ntiles, "plan: %d parts of %d tiles", parts, tpw);
  std::vector<int> tile_owner(ntiles, 0);
  for (int y = 0; y < parts; ++y) {
    const int T0 = y * tpw, T1 = rts_min_i(ntiles, T0 + tpw);
    CHECK(T0 < T1, "empty column range %d", y);
    for (int t = T0; t < T1; ++t) ++tile_owner[t];
  }
  for (int t = 0; t < ntiles; ++t) CHECK(tile_owner[t] == 1, "tile %d in %d ranges", t, tile_owner[t]);
  // units of 4 floats: who read the gu unit, who wrote the dgu unit (workgroup-wave-lane-step id + 1), and how often
  const size_t units = (size_t)(M * ldc / 4);
  std::vector<unsigned char> rd_cnt(units, 0), wr_cnt(units, 0);
  std::vector<uint32_t> rd_who(units, 0);
  int64_t mismatched = 0;
  // pass 0: the gu loads (gu_ld of the kernel, step j of tile t); pass 1: the dgu stores (store_bwd, the same j and t)
  for (int pass = 0; pass < 2; ++pass)
  for (int64_t bx = 0; bx < row_blocks; ++bx)
    for (int y = 0; y < parts; ++y) {
      const int T0 = y * tpw, T1 = rts_min_i(ntiles, T0 + tpw);
      for (int wave = 0; wave < 8; ++wave) {
        const int64_t m0 = (bx * 8 + wave) * 32;
        for (int lane = 0; lane < 64 && pass == 0; ++lane) {
          const int64_t r = rts_a_row(m0, lane & 31, M);
          CHECK(r >= 0 && r < M, "A row");
          for (int s = 0; s < RTS_KS; ++s) CHECK(rts_a_col(s, lane >> 5) + 8 <= K && r * lda + rts_a_col(s, lane >> 5) + 8 <= M * lda, "A element");
        }
        for (int t = T0; t < T1; ++t)
          for (int j = 0; j < 4; ++j)
            for (int grp = 0; grp < 8; ++grp) {
              // the eight lanes 8 grp .. 8 grp + 7 of one load / store instruction: one row, one aligned 128-byte line per stream
              const int64_t row = m0 + rts_st_row(8 * grp, j);
              for (int half = 0; half < 2; ++half) {
                const int c0 = half ? rts_bwd_up_col(t, rts_st_col(8 * grp), F) : rts_bwd_gate_col(t, rts_st_col(8 * grp));
                const int64_t first = row * ldc + c0;
                CHECK(first % 32 == 0, "line of row %lld column %d not aligned", (long long)row, c0);
                for (int l8 = 0; l8 < 8; ++l8) {
                  const int lane = 8 * grp + l8;
                  CHECK(m0 + rts_st_row(lane, j) == row, "eight lanes on two rows");
                  const int col = half ? rts_bwd_up_col(t, rts_st_col(lane), F) : rts_bwd_gate_col(t, rts_st_col(lane));
                  CHECK(row * ldc + col == first + 4 * l8, "lane %d off its place in the line", lane);
                  CHECK(col % 4 == 0 && col + 4 <= 2 * F && (half ? col >= F : col + 4 <= F), "column %d", col);
                  if (row >= M) continue;                                 // GUARD: neither read nor written
                  const size_t u = (size_t)((row * ldc + col) / 4);
                  const uint32_t who = (uint32_t)(((bx * parts + y) * 8 + wave) * 64 + lane) * 4u + (uint32_t)j + 1u;
                  if (pass == 0) { ++rd_cnt[u]; rd_who[u] = who; }
                  else { ++wr_cnt[u]; mismatched += rd_who[u] != who; }   // the store: by the lane and step that read gu there
                }
              }
            }
      }
    }
  int64_t bad = 0;
  for (size_t i = 0; i < units; ++i) bad += (rd_cnt[i] != 1) + (wr_cnt[i] != 1);
  CHECK(bad == 0, "%lld units of gu / dgu not read / written exactly once", (long long)bad);
  CHECK(mismatched == 0, "%lld dgu units written by a lane that did not read their gu", (long long)mismatched);
  // largest byte offset beside the wave's base (32-bit in the kernel)
  CHECK(4 * (31 * ldc + F + 32) < (int64_t)1 << 31, "lane offset");
  if (!g_fail)
    printf("dh + SwiGLU backward M %lld F %d: %d tiles in %d ranges, every gu element read once and every dgu element written once\n",
           (long long)M, F, ntiles, parts);
}

// ---- the A prologue by whole lines (every form): kind 1 gate | up (NF = F), 2 dh + SwiGLU backward (NF = F), 3 q | k | v (NF = D)
static void check_prologue(int kind, int64_t M, int NF) {
  const int K = RTS_K, ntiles = kind == 1 ? NF / 16 : kind == 2 ? NF / 32 : 3 * NF / 32;
  const int64_t lda = K, ldxn = K;
  CHECK(RTS_CHUNKS * 32 == K && RTS_CHUNKS * 2 == RTS_KS, "chunks");
  // the staging round trip of a chunk: what the fragment read of lane (li, lh), k-step parity e, half finds
  {
    std::vector<int> row(RTS_STG / 16, -1), col(RTS_STG / 16, -1);
    for (int i = 0; i < 4; ++i)
      for (int g8 = 0; g8 < 8; ++g8) {
        int banks[32] = {0};                                               // ds_write_b128: eight contiguous lanes, 32 banks
        for (int l8 = 0; l8 < 8; ++l8) {
          const int lane = 8 * g8 + l8, off = rts_pl_stg_w(lane, i);
          CHECK(off >= 0 && off + 16 <= RTS_STG && off % 16 == 0, "chunk write %d", off);
          CHECK(3 * RTS_TILE + 7 * RTS_STG + off + 16 <= RTS_LDS, "staging area past the allocation");
          CHECK(row[off / 16] < 0, "chunk unit written twice");
          row[off / 16] = rts_pl_row(lane, i); col[off / 16] = rts_pl_col(lane, 0);
          for (int d = 0; d < 4; ++d) ++banks[(off / 4 + d) & 31];
        }
        for (int bk = 0; bk < 32; ++bk) CHECK(banks[bk] <= 2, "%d lanes on a bank in a chunk write", banks[bk]);
      }
    // ds_read_b128: four groups of sixteen lanes, 64 banks
    static const int grp[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                   {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    for (int e = 0; e < 2; ++e)
      for (int half = 0; half < 2; ++half) {
        for (int g = 0; g < 4; ++g) {
          int banks[64] = {0};
          for (int q = 0; q < 16; ++q) {
            const int lane = grp[g][q], off = rts_pl_stg_r(lane & 31, lane >> 5, e, half);
            for (int d = 0; d < 4; ++d) ++banks[(off / 4 + d) & 63];
          }
          for (int bk = 0; bk < 64; ++bk) CHECK(banks[bk] <= 2, "%d lanes on a bank in a fragment read", banks[bk]);
        }
        for (int lane = 0; lane < 64; ++lane) {
          const int li = lane & 31, lh = lane >> 5, off = rts_pl_stg_r(li, lh, e, half);
          CHECK(off >= 0 && off + 16 <= RTS_STG && off % 16 == 0, "fragment read %d", off);
          for (int c = 0; c < RTS_CHUNKS; ++c) {
            // the fragment of k-step s = 2 c + e wants k = rts_a_col(s, lh) + 4 half .. + 3 of row li
            CHECK(row[off / 16] == li && 32 * c + col[off / 16] == rts_a_col(2 * c + e, lh) + 4 * half, "lane (%d, %d) k-step %d half %d finds row %d column %d",
                  li, lh, 2 * c + e, half, row[off / 16], 32 * c + col[off / 16]);
          }
        }
      }
    // the rows' statistics: written by the lanes (lane & 7) == 0, one place per row, read by the row's fragment lanes
    std::vector<int> srow(32, 0);
    for (int lane = 0; lane < 64; lane += 8)
      for (int i = 0; i < 4; ++i) {
        const int off = rts_pl_stat(rts_pl_row(lane, i));
        CHECK(off >= 0 && off + 8 <= RTS_STG && off % 8 == 0 && off == 16 * rts_pl_row(lane, i), "statistics place %d", off);
        ++srow[rts_pl_row(lane, i)];
      }
    for (int r = 0; r < 32; ++r) CHECK(srow[r] == 1, "statistics of row %d written %d times", r, srow[r]);
  }
  int tpw, parts;
  rts_plan(M, ntiles, &tpw, &parts);
  const int64_t row_blocks = (M + 255) / 256;
  std::vector<unsigned char> xn_cnt((size_t)(M * ldxn), 0), rms_cnt((size_t)M, 0);
  std::vector<unsigned char> seen(32 * K);
  for (int64_t bx = 0; bx < row_blocks; ++bx)
    for (int y = 0; y < parts; ++y)
      for (int wave = 0; wave < 8; ++wave) {
        const int64_t m0 = (bx * 8 + wave) * 32;
        std::fill(seen.begin(), seen.end(), 0);
        for (int c = 0; c < RTS_CHUNKS; ++c)
          for (int i = 0; i < 4; ++i)
            for (int g8 = 0; g8 < 8; ++g8) {
              // one load instruction = eight groups of eight lanes, each on one aligned 128-byte line of one row
              const int rl = rts_pl_row(8 * g8, i);
              const int64_t r = rts_a_row(m0, rl, M), first = r * lda + rts_pl_col(8 * g8, c);
              CHECK(r >= 0 && r < M && first % 32 == 0, "line of row %lld", (long long)r);
              for (int l8 = 0; l8 < 8; ++l8) {
                const int lane = 8 * g8 + l8;
                CHECK(rts_pl_row(lane, i) == rl && r * lda + rts_pl_col(lane, c) == first + 4 * l8, "lane %d off its line", lane);
                CHECK(rts_pl_col(lane, c) + 4 <= K && r * lda + rts_pl_col(lane, c) + 4 <= M * lda, "A element");
                for (int d = 0; d < 4; ++d) ++seen[rl * K + rts_pl_col(lane, c) + d];
                if (y == 0 && m0 + rl < M && kind != 2)                    // xn: the first column range, rows inside the matrix
                  for (int d = 0; d < 4; ++d) ++xn_cnt[(size_t)((m0 + rl) * ldxn + rts_pl_col(lane, c) + d)];
              }
            }
        for (int e = 0; e < 32 * K; ++e) CHECK(seen[e] == 1, "A element %d of a wave read %d times", e, seen[e]);
        for (int lane = 0; lane < 32; ++lane)                                // rms: lanes lh == 0
          if (y == 0 && m0 + lane < M && kind != 2) ++rms_cnt[(size_t)(m0 + lane)];
      }
  int64_t bad = 0;
  if (kind != 2) {
    for (size_t i = 0; i < xn_cnt.size(); ++i) bad += xn_cnt[i] != 1;
    for (size_t i = 0; i < rms_cnt.size(); ++i) bad += rms_cnt[i] != 1;
  }
  CHECK(bad == 0, "%lld elements of xn / rms not written exactly once", (long long)bad);
  if (!g_fail) printf("prologue kind %d M %lld NF %d: %d ranges, every A element read once by whole lines, xn and rms written once\n", kind, (long long)M, NF, parts);
}

int main(int argc, char** argv) {
  // arguments: "b M F" = the dh + SwiGLU backward form; "p kind M NF" = the A prologue of form `kind`
  int i = 1;
  if (argc < 2) { printf("usage: %s [b M F | p kind M NF] ...\n", argv[0]); return 2; }
  while (i < argc) {
    if (!strcmp(argv[i], "b") && i + 2 < argc) { check_shape(atoll(argv[i + 1]), atoi(argv[i + 2])); i += 3; }
    else if (!strcmp(argv[i], "p") && i + 3 < argc) { check_prologue(atoi(argv[i + 1]), atoll(argv[i + 2]), atoi(argv[i + 3])); i += 4; }
    else { printf("usage: %s [b M F | p kind M NF] ...\n", argv[0]); return 2; }
    if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  }
  return 0;
}
