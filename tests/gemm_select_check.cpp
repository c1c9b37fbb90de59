// Stand-alone program around pydynet_amd/csrc/gemm_select.h, the host-only header in which pdn_gemm_f32 (csrc/gemm.hip)
// decides between the wave-streaming and the tiled kernel, their tile shape and their k-split.  Given the numbers of a call
// that reaches that choice it prints the line the library prints under PDN_GEMM_DEBUG, from the same formatter; the routing
// variables (PDN_GEMM_CFG, PDN_GEMM_STREAM_*, PDN_GEMM_NO_STREAM, PDN_GEMM_NO_FIXED) are read from the environment as the
// library reads them.  Built and run by tests/test_gemm_select_cpu.py with the host compiler under AddressSanitizer and
// UndefinedBehaviorSanitizer; no HIP header, no GPU.
//
//   gemm_select_check M N K nb1 nb2  a_rs a_cs b_rs b_cs  a_bs1 a_bs2 b_bs1 b_bs2  a_low b_low  ws_bytes  ext_on colsum mask_colsum
//
// a_low / b_low: the low bits of the operands' addresses; ws_bytes: the workspace passed (0: none); ext_on: a mask epilogue
// (pdn_linear_relu_fwd_f32 / pdn_linear_dx_masked_f32); colsum: b_colsum given; mask_colsum: the partial column sums asked for.
#include "../pydynet_amd/csrc/gemm_select.h"

int main(int argc, char** argv) {
  if (argc != 20) {
    fprintf(stderr, "usage: %s M N K nb1 nb2 a_rs a_cs b_rs b_cs a_bs1 a_bs2 b_bs1 b_bs2 a_low b_low ws_bytes ext_on colsum mask_colsum\n", argv[0]);
    return 2;
  }
  int64_t v[19];
  for (int i = 0; i < 19; ++i) v[i] = atoll(argv[i + 1]);
  const int M = (int)v[0], N = (int)v[1], K = (int)v[2], nbatch = (int)(v[3] * v[4]);
  const int64_t a_rs = v[5], a_cs = v[6], b_rs = v[7], b_cs = v[8], ws_bytes = v[15];
  if (M <= 0 || N <= 0 || K < 0 || nbatch <= 0) {
    fprintf(stderr, "an empty or negative extent has no route\n");
    return 2;
  }
  const GemmLayout lay = gemm_layout(M, N, K, a_rs, a_cs, b_rs, b_cs, v[9], v[10], v[11], v[12], (uintptr_t)v[13], (uintptr_t)v[14]);
  const GemmChoice ch = gemm_select(M, N, K, nbatch, a_rs, b_cs, lay, v[16] != 0, v[17] != 0, v[18] != 0, ws_bytes > 0 ? ws_bytes / 4 : 0);
  if (ch.cfg < 0) {
    fprintf(stderr, "no tile configuration\n");
    return 1;
  }
  char line[256];
  gemm_route_line(line, sizeof(line), M, N, K, nbatch, lay, ch);
  fputs(line, stdout);
  return 0;
}
