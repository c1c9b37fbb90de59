// Host replay of the RMSNorm-backward drain of the split-fp16 output-resident product (ors_main_kernel<0, 1> of
// pydynet_amd/csrc/outres_split.hip), through the index functions of pydynet_amd/csrc/outres_split_index.h that the kernel
// uses: for every workgroup of the persistent grid, every block it walks, every wave, lane and tile,
//   - the row x / rms are read from lies inside [0, M) (rows past the end read the last row),
//   - every element of dx of every row < M is written exactly once and no row >= M is touched,
//   - the LDS float a lane adds a weight-gradient sum to lies in its own wave's row and inside the allocation, every float of
//     the eight rows is reached, and the partial row a workgroup leaves lies inside [0, ors_grid(M)) x 288.
// usage: normgrad_drain_check M [M ...]      (built with -fsanitize=address,undefined by tests/test_normgrad_drain_check_cpu.py)
#include "../pydynet_amd/csrc/outres_split_index.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define REQUIRE(cond, ...)                     \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAILED: " __VA_ARGS__);     \
      std::printf("  [%s]\n", #cond);          \
      return 1;                                \
    }                                          \
  } while (0)

static int check(int64_t M) {
  const int nblk = ors_blocks(M), grid = ors_grid(M);
  std::vector<unsigned char> dx((size_t)M * ORS_N, 0);          // sized to M rows exactly: a row >= M is out of bounds
  std::vector<unsigned char> part((size_t)grid * ORS_N, 0);
  std::vector<int> visited(nblk, 0);
  for (int wg = 0; wg < grid; ++wg) {
    std::vector<int> lds(ORS_NORM_FLOATS, -1);                 // which wave adds to a float of the epilogue's LDS
    int blk = wg;
    for (;;) {
      REQUIRE(blk < nblk, "workgroup %d walks block %d of %d\n", wg, blk, nblk);
      ++visited[blk];
      for (int wave = 0; wave < 8; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
          const int r = lane & 15, q = lane >> 4;
          const int64_t row = ors_lane_row(blk, wave, r);
          const int64_t rowc = ors_min_l(row, M - 1);
          REQUIRE(rowc >= 0 && rowc < M, "row %lld read for row %lld of %lld\n", (long long)rowc, (long long)row, (long long)M);
          for (int j = 0; j < ORS_NT; ++j) {
            const int col = ors_out_col(j, q);
            REQUIRE(col >= 0 && col + 3 < ORS_N, "column %d\n", col);
            if (row < M)
              for (int e = 0; e < 4; ++e) {
                const size_t at = (size_t)row * ORS_N + col + e;
                REQUIRE(at < dx.size(), "dx element %zu of %zu\n", at, dx.size());
                REQUIRE(dx[at] == 0, "dx row %lld column %d written twice\n", (long long)row, col + e);
                dx[at] = 1;
              }
            if (r == 0)
              for (int e = 0; e < 4; ++e) {
                const int at = ORS_N + ors_dw_lds(wave, col + e);
                REQUIRE(at >= ORS_N && at < ORS_NORM_FLOATS, "LDS float %d of %d\n", at, ORS_NORM_FLOATS);
                REQUIRE(lds[at] == -1 || lds[at] == wave, "LDS float %d shared by waves %d and %d\n", at, lds[at], wave);
                lds[at] = wave;
              }
          }
        }
      const int nxt = ors_next_block(blk, grid, nblk);
      if (nxt == blk) break;
      blk = nxt;
    }
    for (int i = ORS_N; i < ORS_NORM_FLOATS; ++i) REQUIRE(lds[i] == (i - ORS_N) / ORS_N, "LDS float %d belongs to wave %d\n", i, lds[i]);
    for (int c = 0; c < ORS_N; ++c) {
      const size_t at = (size_t)wg * ORS_N + c;
      REQUIRE(at < part.size() && part[at] == 0, "partial element %zu\n", at);
      part[at] = 1;
    }
  }
  for (int b = 0; b < nblk; ++b) REQUIRE(visited[b] == 1, "block %d visited %d times\n", b, visited[b]);
  for (size_t i = 0; i < dx.size(); ++i) REQUIRE(dx[i] == 1, "dx element %zu never written\n", i);
  for (size_t i = 0; i < part.size(); ++i) REQUIRE(part[i] == 1, "partial element %zu never written\n", i);
  std::printf("M = %lld: %d blocks on %d workgroups, every row of dx written once, LDS rows disjoint\n", (long long)M, nblk, grid);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: %s M [M ...]\n", argv[0]); return 2; }
  for (int i = 1; i < argc; ++i)
    if (check(std::atoll(argv[i]))) return 1;
  return 0;
}
