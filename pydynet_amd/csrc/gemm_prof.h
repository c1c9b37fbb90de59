// Optional per-launch timing of the GEMM kernels (bench.py roofline), defined in csrc/gemm.hip: a launch between `begin`
// and `end` is timed under a kernel family when profiling is on (pdn_gemm_prof_enable); with profiling off nothing is
// created or recorded.  Not part of the C ABI.
#pragma once

// token = index + 1 of the open record, 0 when profiling is off
int pdn_gemm_prof_begin(int family, double flops, double bytes, void* stream);
void pdn_gemm_prof_end(int token, void* stream);

// `begin` where it is declared, `end` where its scope is left -- on an error return too, so that no record stays without
// its closing event
struct GemmProfScope {
  GemmProfScope(int family, double flops, double bytes, void* stream)
      : stream_(stream), token_(pdn_gemm_prof_begin(family, flops, bytes, stream)) {}
  ~GemmProfScope() { pdn_gemm_prof_end(token_, stream_); }
  GemmProfScope(const GemmProfScope&) = delete;
  GemmProfScope& operator=(const GemmProfScope&) = delete;

 private:
  void* stream_;
  int token_;
};
