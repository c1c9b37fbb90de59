// Host restatement of the global accesses of stn_split_xn_kernel (pydynet_amd/csrc/split_tn_planes.hip): the plane pass that
// forms an RMSNorm output from (x, rms, w) on the way into the fp16 plane images, with every index taken from
// pydynet_amd/csrc/split_tn_index.h as the kernel takes it.  Over every workgroup, thread and load of K tokens:
//   * x: nine 16-byte loads per thread, each inside the (K x 288) matrix, every 16 bytes of it read exactly once;
//   * rms: thread t < 32 of workgroup b reads rms[32 b + t]: inside its K floats, each read once;
//   * w: columns d < 288 only; xsh: written by workgroup 0 alone, 288 ints right behind the images, inside the extra region;
//   * the image: staged through LDS and read back unit by unit, the 36 KiB of piece b hold, at byte 2 (8 u + k) of plane h and
//     of plane l, token 32 b + 8 q + k of column d with (d, q) = stn_pass_unit_d / _q (u) -- the very bytes the old pass
//     (stn_split_x_kernel on a written xn) puts there, which is restated beside it from stn_x_unit and compared.
// Values are element numbers (token * 288 + column), so that a wrong address shows as a wrong number whatever the arithmetic.
// usage: norm_planes_check K [K ...]      (built with -fsanitize=address,undefined by tests/test_norm_planes_check_cpu.py)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pydynet_amd/csrc/split_tn_index.h"

#define CHECK(c, msg)                                                       \
  do {                                                                      \
    if (!(c)) { std::printf("FAILED: %s (%s:%d)\n", msg, __FILE__, __LINE__); return 1; } \
  } while (0)

static int run(int64_t K) {
  CHECK(K % STN_KP == 0 && K >= OTS_MIN_K, "K as the split route takes it");
  const int64_t ldx = STN_N, npieces = K / STN_KP;
  const int64_t x_floats = K * ldx, extra = stn_extra_bytes(K, OTS_XKIB);
  std::vector<uint8_t> x_read(x_floats / 4, 0), rms_read(K, 0);
  std::vector<int64_t> raw(STN_KP * STN_N), img_new(stn_xpiece(OTS_XKIB) / 2), img_old(stn_xpiece(OTS_XKIB) / 2);
  int xsh_written[STN_N] = {0};
  for (int64_t b = 0; b < npieces; ++b) {
    // ---- loads: x staged raw, rms by the first 32 threads, the exponents by workgroup 0
    for (auto& v : raw) v = -1;
    for (int tid = 0; tid < STN_PASS_THREADS; ++tid) {
      for (int e = 0; e < STN_PASS_LOADS; ++e) {
        const int i = tid + STN_PASS_THREADS * e;
        const int64_t src = b * STN_KP * ldx + (int64_t)stn_pass_row(i) * ldx + 4 * stn_pass_chunk(i);
        CHECK(src >= 0 && src + 4 <= x_floats && src % 4 == 0, "x load outside the matrix or off 16 bytes");
        CHECK(++x_read[src / 4] == 1, "16 bytes of x read twice");
        for (int j = 0; j < 4; ++j) {
          const int a = stn_pass_lds(stn_pass_row(i), 4 * stn_pass_chunk(i)) + j;
          CHECK(a >= 0 && a < STN_KP * STN_N && raw[a] == -1, "LDS staging outside the array or written twice");
          raw[a] = src + j;
        }
      }
      if (tid < STN_KP) {
        const int64_t r = b * STN_KP + tid;
        CHECK(r < K && ++rms_read[r] == 1, "rms read outside its K floats or twice");
      }
      if (b == 0)
        for (int d = tid; d < STN_N; d += STN_PASS_THREADS) {
          const int64_t at = npieces * stn_xpiece(OTS_XKIB) + 4 * (int64_t)d;
          CHECK(at + 4 <= extra && ++xsh_written[d] == 1, "exponent outside the extra region or written twice");
        }
    }
    // ---- stores: the new pass from its LDS, the old pass's image restated from stn_x_unit
    for (auto& v : img_new) v = -1;
    for (int tid = 0; tid < STN_PASS_THREADS; ++tid)
      for (int e = 0; e < (STN_N * 4 + STN_PASS_THREADS - 1) / STN_PASS_THREADS; ++e) {
        const int u = tid + STN_PASS_THREADS * e;
        if (u >= STN_N * 4) continue;
        const int d = stn_pass_unit_d(u), q = stn_pass_unit_q(u);
        CHECK(d < STN_N, "w read outside its 288 floats");
        CHECK(16 * u + 16 <= STN_PLANE, "unit outside its plane");
        for (int k = 0; k < 8; ++k) {
          CHECK(8 * q + k < STN_KP, "1 / rms read outside the piece's 32 values");
          const int64_t v = raw[stn_pass_lds(8 * q + k, d)];
          CHECK(img_new[8 * u + k] == -1, "image half written twice");
          img_new[8 * u + k] = v;                            // plane h at halves 8 u + k, plane l the same halves further on
          img_new[STN_PLANE / 2 + 8 * u + k] = v;
        }
      }
    for (int d = 0; d < STN_N; ++d)
      for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 8; ++k) {
          const int64_t v = (b * STN_KP + 8 * q + k) * ldx + d;
          img_old[stn_x_unit(d, q) / 2 + k] = v;
          img_old[STN_PLANE / 2 + stn_x_unit(d, q) / 2 + k] = v;
        }
    CHECK(img_new == img_old, "the image differs from the old pass's");
  }
  for (auto c : x_read) CHECK(c == 1, "16 bytes of x never read");
  for (auto c : rms_read) CHECK(c == 1, "an rms never read");
  for (int d = 0; d < STN_N; ++d) CHECK(xsh_written[d] == 1, "an exponent never written");
  std::printf("K = %lld: %lld workgroups, every 16 bytes of x and every rms read once inside their buffers, the exponents behind "
              "the images, every image equal to the old pass's\n", (long long)K, (long long)npieces);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: norm_planes_check K [K ...]\n"); return 2; }
  for (int i = 1; i < argc; ++i)
    if (run(std::atoll(argv[i]))) return 1;
  return 0;
}
