// What pdn_gemm_f32 (csrc/gemm.hip) decides on the host for the products that reach its last route, the wave-streaming
// weight-gradient kernels (csrc/gemm_stream.h) or the tiled kernel (csrc/gemm_tiled.h): the LDS layout of the operands, the
// streaming tile shape and its k-split, the tile configuration and its k-split, and the line PDN_GEMM_DEBUG prints.  Pure
// arithmetic on extents, strides, the low bits of the addresses, the workspace size and the routing variables of the
// environment (read on every call), and host-only: no HIP header, so tests/gemm_select_check.cpp builds it with the host
// compiler and prints the route of a call without a GPU.  The launches stay in csrc/gemm.hip and switch on GemmChoice.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>

struct TileCfg {
  int waves_m, waves_n, wm, wn, bk;
  float eff;  // relative efficiency of the tile shape (operand bytes per MFMA, barrier rate)
};
static const TileCfg kCfgs[] = {
    // eff values are fitted to the round-1 tile sweep on MI355X (tools/gemm_bench.py, profiles/)
    {2, 2, 2, 2, 32, 1.00f},  // 0: 128 x 128
    {4, 1, 1, 3, 32, 0.97f},  // 1: 128 x  96   (N = 288 = 3*96)
    {1, 4, 3, 1, 32, 0.95f},  // 2:  96 x 128   (M = 288, weight gradients)
    {4, 1, 1, 2, 32, 0.85f},  // 3: 128 x  64
    {1, 4, 2, 1, 32, 0.90f},  // 4:  64 x 128
    {2, 2, 1, 1, 32, 0.60f},  // 5:  64 x  64
    {2, 2, 4, 2, 16, 0.85f},  // 6: 256 x 128
    {2, 2, 2, 4, 16, 1.10f},  // 7: 128 x 256   (only offered to very wide outputs, see below)
    {4, 1, 2, 3, 16, 0.99f},  // 8: 256 x  96
    {1, 4, 3, 2, 16, 0.70f},  // 9:  96 x 256
    {2, 1, 1, 3, 32, 0.78f},  // 10: 64 x  96   (2 waves: finer quantisation for N = 288)
    {1, 2, 3, 1, 32, 0.70f},  // 11: 96 x  64
    {4, 1, 1, 3, 16, 1.15f},  // 12: 128 x 96, BK 16: 51 KB of LDS -> three workgroups per CU (offered selectively)
    // (tried in round 2: {4, 1, 1, 9, 16} = 128 x 288, the whole 288-wide row panel in one workgroup so that the
    //  65536 x 32000 dlogits operand of the lm_head input gradient is read from HBM once instead of 1.76 times
    //  (PMC: FETCH 14.8 GB vs 8.4 GB algorithmic) -- 10.45 ms against 9.79 ms for the 96 x 128 tile: the product is
    //  matrix-pipe bound, the re-reads are L2 / MALL hits that cost nothing; not kept)
};
static const int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);
static const int kScalarCfg = 5;

constexpr int kStreamWaves = 8;                          // waves per streaming workgroup
// tile shape of the LDS-staged streaming kernel (in 32-row / 32-column MFMA tiles): 3 x 3 unless another one pads the output
// less (784 x 1024: 9 x 11 tiles of 96 x 96 = 912 K accumulators, 5 x 16 of 160 x 64 = 819 K)
static const int kShapes[5][2] = {{3, 3}, {5, 2}, {2, 5}, {4, 2}, {2, 4}};
// time per accumulator of the padded output relative to 3 x 3 (tools/mlp_dw_probe.py, 65536 tokens: 784 x 1024,
// 1024 x 1024, 768 x 768, 512 x 2048); an exact 3 x 3 tiling takes the DMA-staged kernel
static const double kShapeCost[5] = {1.0, 1.05, 1.08, 1.07, 1.02};
static const int kPadTiles[3][2] = {{128, 128}, {128, 96}, {96, 128}};

// the streaming kernel a launch picks: DMA-staged, LDS-staged (exact 3 x 3 tiling / with edge tests), or dword loads
// without LDS (unaligned operands, PDN_GEMM_STREAM_DIRECT)
enum GemmStreamKind { kStreamDma = 0, kStreamLds, kStreamLdsEdge, kStreamDirect, kStreamDirectEdge };
static const char* const kStreamKindNames[5] = {"dma", "lds", "lds-edge", "direct", "direct-edge"};

static inline int64_t gemm_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool gemm_al16(uintptr_t addr) { return (addr & 15) == 0; }
static inline bool gemm_m4(int64_t v) { return (v & 3) == 0; }

struct GemmLayout {
  bool a_kin, b_kin;   // LDS layout per operand: contraction-contiguous (KIN) unless the m/n index is the unit stride
  bool vec;            // the float4 path
};

static inline GemmLayout gemm_layout(int M, int N, int K, int64_t a_rs, int64_t a_cs, int64_t b_rs, int64_t b_cs,
                                     int64_t a_bs1, int64_t a_bs2, int64_t b_bs1, int64_t b_bs2, uintptr_t a_addr,
                                     uintptr_t b_addr) {
  GemmLayout l;
  l.a_kin = !(a_rs == 1 && a_cs != 1) || M == 1;
  l.b_kin = (b_rs == 1 && b_cs != 1) || (b_rs == 1 && N == 1);
  // float4 path: unit stride on the staged-contiguous index, every row start 16B aligned,
  // extents along the contiguous index multiples of 4.
  bool vec = gemm_al16(a_addr) && gemm_al16(b_addr) && gemm_m4(a_bs1) && gemm_m4(a_bs2) && gemm_m4(b_bs1) && gemm_m4(b_bs2);
  if (l.a_kin) vec = vec && a_cs == 1 && gemm_m4(a_rs) && gemm_m4(K);
  else vec = vec && a_rs == 1 && gemm_m4(a_cs) && gemm_m4(M);
  if (l.b_kin) vec = vec && b_rs == 1 && gemm_m4(b_cs) && gemm_m4(K);
  else vec = vec && b_cs == 1 && gemm_m4(b_rs) && gemm_m4(N);
  l.vec = vec;
  return l;
}

struct GemmChoice {
  bool use_stream;
  int cfg;             // index into kCfgs (0 for a streamed product); -1: no tile configuration
  int cost_splits;     // tiled: the k-split the model or PDN_GEMM_CFG asked for (what the route line prints)
  int splits;          // slabs really written: cdiv(K, k_per_split)
  int k_per_split;
  int tiles_m, tiles_n;
  int sshape;          // streamed: index into kShapes
  GemmStreamKind kind; // streamed: the kernel variant
};

// `ext_on`: a mask epilogue (no k-split, the tile shapes built with MASKS); `colsum`: fused column sums (no k-split);
// `mask_colsum`: the 32-row partial column sums of the masked input gradient; `ws_cap`: workspace capacity in floats.
static inline GemmChoice gemm_select(int M, int N, int K, int nbatch, int64_t a_rs, int64_t b_cs, const GemmLayout& lay,
                                     bool ext_on, bool colsum, bool mask_colsum, int64_t ws_cap) {
  const bool a_kin = lay.a_kin, b_kin = lay.b_kin, vec = lay.vec;
  GemmChoice ch;
  ch.use_stream = false; ch.cfg = -1; ch.cost_splits = 1; ch.splits = 1; ch.k_per_split = 0; ch.tiles_m = ch.tiles_n = 0;
  ch.sshape = 0; ch.kind = kStreamDma;
  // ---- weight-gradient form (small output, long K): wave-streaming kernel --------------------
  constexpr int SNW = kStreamWaves;
  bool use_stream = false;
  int sshape = 0;
  // Which weight gradients it takes (tools/gemm_fc_sweep.py, same process, warm clocks, K = 4096 ... 65536):
  //   * outputs BELOW 2^20 elements: at 1024 x 1024 -- config 2's second layer -- the tiled kernel with its k-split measured
  //     1065 us against 1144 us, and the MLP step 5.44 -> 5.32 ms (PDN_GEMM_STREAM_MAX overrides the bound);
  //   * from 2^18 elements on only where the tiled kernel's 128 / 96-wide tiles would PAD the output by more than 4 %:
  //     784 x 1024 (config 2's first layer: 9 x 8 tiles of 96 x 128 = +10 %) 954 us here against 1030-1080 us tiled, but
  //     512 x 512 and 512 x 1536 (the Transformer example, the dim-512 Llama) 38 / 85 us tiled against 45 / 109 us here at
  //     K = 5632 and 280 / 804 against 330 / 890 us at K = 65536; below 2^18 (288 x 288, 288 x 768) this kernel wins at every K.
  bool stream_fits = (int64_t)M * N * nbatch <= (getenv("PDN_GEMM_STREAM_MAX") ? atol(getenv("PDN_GEMM_STREAM_MAX")) : (1 << 20) - 1);
  if (stream_fits && (int64_t)M * N * nbatch >= (1 << 18) && !getenv("PDN_GEMM_STREAM_MAX")) {
    double pad = 1e30;
    for (const auto& t : kPadTiles)
      pad = std::min(pad, (double)(gemm_cdiv(M, t[0]) * t[0]) * (double)(gemm_cdiv(N, t[1]) * t[1]) / ((double)M * N));
    stream_fits = pad > 1.04;
  }
  if (!ext_on && !a_kin && !b_kin && a_rs == 1 && b_cs == 1 && !colsum && K >= 2048 && stream_fits && nbatch <= 64 &&
      !getenv("PDN_GEMM_NO_STREAM")) {
    sshape = 0;
    if (vec) {
      double best_area = (double)gemm_cdiv(M, 96) * gemm_cdiv(N, 96) * 96 * 96 * ((M % 96 == 0 && N % 96 == 0) ? 0.975 : 1.0);
      for (int c = 1; c < 5; ++c) {
        const int th = kShapes[c][0] * 32, tw = kShapes[c][1] * 32;
        const double area = (double)gemm_cdiv(M, th) * gemm_cdiv(N, tw) * th * tw * kShapeCost[c];
        if (area < best_area) { best_area = area; sshape = c; }
      }
      if (const char* e = getenv("PDN_GEMM_STREAM_SHAPE")) { const int c = atoi(e); if (c >= 0 && c < 5) sshape = c; }
    }
    const int sth = kShapes[sshape][0] * 32, stw = kShapes[sshape][1] * 32;
    const int tm = (int)gemm_cdiv(M, sth), tn = (int)gemm_cdiv(N, stw), tiles = tm * tn * nbatch;
    if (tiles <= 256) {
      // one 8-wave workgroup per CU (2 waves / SIMD): rounds of 256 blocks; each extra slab costs a
      // write + read of the output in the reduce pass (~1.7 KB/clk), plus its launch
      double best_cost = 1e300;
      int best_kps = 0, best_sp = 1;
      const int smax = (int)std::min<int64_t>(64, K / (SNW * 16));
      for (int s = 1; s <= smax; ++s) {
        if (s > 1 && (int64_t)s * M * N * nbatch > ws_cap) break;
        const int kw = (int)gemm_cdiv(gemm_cdiv(K, (int64_t)s * SNW), 8) * 8;
        const int kps = kw * SNW, sp = (int)gemm_cdiv(K, kps);
        const double rounds = (double)gemm_cdiv((int64_t)tiles * sp, 256);
        double cost = rounds * (kw * 0.5 * (kShapes[sshape][0] * kShapes[sshape][1]) * 64 * (SNW / 4.0) + 6000.0);
        if (sp > 1) cost += (double)sp * M * N * nbatch * 8.0 / 1700.0 + 5000.0;
        if (cost < best_cost) { best_cost = cost; best_kps = kps; best_sp = sp; }
      }
      if (const char* e = getenv("PDN_GEMM_STREAM_SPLITS")) {     // tuning override
        const int s = atoi(e);
        if (s >= 1 && (s == 1 || (int64_t)s * M * N * nbatch <= ws_cap)) {
          const int kw = (int)gemm_cdiv(gemm_cdiv(K, (int64_t)s * SNW), 8) * 8;
          best_kps = kw * SNW; best_sp = (int)gemm_cdiv(K, best_kps);
        }
      }
      use_stream = true;
      ch.tiles_m = tm; ch.tiles_n = tn; ch.k_per_split = best_kps; ch.splits = best_sp;
    }
  }

  // ---- pick tile shape and k-split with a small cost model -----------------------------
  // The matrix pipes of a CU are shared by its resident workgroups, so MFMA throughput is
  // counted per CU (256), not per residency slot: n blocks take ceil(n/256) block-times until
  // the grid is large enough (>= 4 rounds) for the dispatcher to even the load out.
  int best = -1, best_splits = 1;
  double best_cost = 1e300;
  static const bool no_fixed = getenv("PDN_GEMM_NO_FIXED") != nullptr;      // A/B switch for the residency-round term
  for (int c = 0; c < kNumCfgs && !use_stream; ++c) {
    if (!vec && c != kScalarCfg) continue;  // scalar staging: 64x64 only
    if (ext_on && !(c == 0 || c == 3 || c == 6 || c == 7 || c == 8 || c == kScalarCfg)) continue;   // the tile shapes built with MASKS
    if (mask_colsum && c == 8) continue;    // (a lane keeps its columns over a band only when 64 % (8 WN) == 0)
    // 128 x 256: very wide outputs -- and (round 6) the 1024-wide Linear + ReLU layers of config 2 at chip-filling row
    // counts, where it measures 0.86 of the fp32-MFMA peak against 0.71-0.80 for 128 x 128 (tools/gemm_fc_sweep.py)
    if (c == 7 && N < 2048 && !(ext_on && N >= 1024 && N % 256 == 0 && M >= 16384)) continue;
    if (c == 6 && ext_on && !(N >= 1024 && M >= 16384)) continue;
    if (c == 8 && N < 768) continue;        // 256-row tiles lose on narrow outputs (one block per CU)
    const int BM = kCfgs[c].waves_m * kCfgs[c].wm * 32, BN = kCfgs[c].waves_n * kCfgs[c].wn * 32;
    const int bk = kCfgs[c].bk;
    const int64_t tiles = gemm_cdiv(M, BM) * gemm_cdiv(N, BN) * nbatch;
    // 128x96 with BK 16 keeps THREE workgroups per CU: worth it exactly when two-per-CU would
    // leave a half-empty last round of short blocks (measured: 73 -> 58 us on 32768x288x288)
    if (c == 12 && !(tiles > 512 && tiles <= 768 && K <= 1024 && a_kin && !b_kin)) continue;
    const int ktiles = (int)gemm_cdiv(K > 0 ? K : 1, bk);
    for (int s = 1; s <= 64; s *= 2) {
      if (s > 1 && (colsum || ext_on)) break;
      if (s > 1) {
        if (ktiles * bk / s < 128) break;
        if ((int64_t)s * M * N * nbatch > ws_cap) break;
      }
      const int kps = (int)gemm_cdiv(ktiles, s);
      // Model (fitted to tools/gemm_sweep_dw.py and the tile sweep): a block keeps `waves_pb`
      // SIMDs busy for BM*BN*K/waves_pb MFMA-cycles; blocks are dealt round-robin over the 256
      // CUs, so a grid needs ceil(blocks/slots) rounds until it is large enough to even out; a CU
      // with at least two resident blocks hides their barriers/prologues behind each other
      // (~0.7 -> 1.0 matrix-pipe duty), which is why ~480 blocks beat 240 longer ones.
      const double waves_pb = kCfgs[c].waves_m * kCfgs[c].waves_n;
      const double blocks = (double)tiles * s;
      const double slots = 256.0 * (4.0 / waves_pb);
      const double rounds = blocks >= 4 * slots ? blocks / slots : (double)gemm_cdiv((int64_t)blocks, (int64_t)slots);
      const double wps = blocks * waves_pb / 1024.0;   // resident waves per SIMD in a round
      const double util = wps >= 1.875 ? 1.0 : (wps > 1.0 ? 0.7 + 0.3 * (wps - 1.0) / 0.875 : 0.7);
      const double eff = kCfgs[c].eff;
      double cost = rounds * ((double)BM * BN * (kps * bk + 64) / waves_pb * 4.0 / (eff * util));
      // ... plus what a block costs besides its MFMAs (first tiles in, accumulators out: ~25k cycles = 10 us, fitted at
      // 16384 x 288 x {288, 768, 864}: 38 us for 384 blocks of 128 x 96 against 46 us for 768 of 64 x 128), paid once
      // per RESIDENCY round -- co-resident blocks overlap theirs -- which is what makes few fat blocks win on short
      // products even when they leave CUs half loaded (round 3; the unit is 1/156 matrix-pipe cycle)
      if (!no_fixed) {
        const double per_cu = c == 12 ? 3.0 : 2.0;
        cost += (double)gemm_cdiv((int64_t)blocks, (int64_t)(256.0 * per_cu)) * 3.9e6;
      }
      if (s > 1) cost += (double)M * N * nbatch * (s + 1) * 0.5 + 1.0e6;   // slab pass + extra launch
      if (cost < best_cost) { best_cost = cost; best = c; best_splits = s; }
    }
  }
  if (best < 0 && !use_stream) return ch;                 // (cfg -1: the caller refuses the call)
  if (!use_stream && best_splits == 1 && !colsum && !ext_on && K >= 8192) {
    // 2-4 very long blocks per CU: the last one of each CU runs without a co-resident partner to
    // hide its barriers behind; halving the blocks evens that out (measured -3..4 % on the
    // 32768 x 288 x 32000 and 288 x 32000 x 32768 products, slab pass included)
    const int BMb = kCfgs[best].waves_m * kCfgs[best].wm * 32, BNb = kCfgs[best].waves_n * kCfgs[best].wn * 32;
    const int64_t blocks = gemm_cdiv(M, BMb) * gemm_cdiv(N, BNb) * nbatch;
    if (blocks > 512 && blocks < 1024 && (int64_t)2 * M * N * nbatch <= ws_cap) best_splits = 2;
  }
  // Mid-size products that 128 x 128 tiles cannot spread over the chip (fewer than 256 of them) or whose contraction is
  // short (K <= 512): 64 x 64 tiles with a k-split.  Config 3's fully connected layers (4096 x 3200 x 500 in its three
  // forms) measured inside the step: 1.390 -> 1.335 ms with `5,8` for all of them, every other choice in between
  // (round 6; the cost model above prices a block's fixed cost too high for these).
  // The k-split pays in the weight-gradient form only (long contraction over the rows): with the rows on the output side
  // 5632 x 512 over K = 1536 measured 85 us unsplit against 94 / 96 / 103 us split 2 / 4 / 8 ways, 8192 x 1024 over 1024
  // 143 against 161 / 177 / 233 us (tools/gemm_fc_sweep.py) -- and the Linear + ReLU products (mask epilogues: no split) take
  // the same tiles: 5632 x 512 -> 1536 with its ReLU 104 -> 8x us.
  if (!use_stream && !colsum && vec && nbatch == 1 && (int64_t)M * N >= (1 << 20) && (int64_t)M * N <= (1 << 24) &&
      K <= 4096 && K >= 128 && (gemm_cdiv(M, 128) * gemm_cdiv(N, 128) < 256 || K <= 512)) {
    int sp = (a_kin || ext_on) ? 1 : 8;
    while (sp > 1 && (K / sp < 64 || (int64_t)sp * M * N > ws_cap)) sp >>= 1;
    best = kScalarCfg;
    best_splits = sp;
  }
  if (use_stream) best = 0;
  else if (const char* e = getenv("PDN_GEMM_CFG")) {            // tuning override: "<cfg>[,<splits>]"
    int c = -1, sp = 0;
    if (sscanf(e, "%d,%d", &c, &sp) >= 1 && c >= 0 && c < kNumCfgs && vec &&
        (!ext_on || c == 0 || c == 3 || c == 6 || c == 7 || (c == 8 && !mask_colsum) || c == kScalarCfg)) {
      best = c;
      if (sp >= 1 && (sp == 1 || ((int64_t)sp * M * N * nbatch <= ws_cap && !colsum && !ext_on))) best_splits = sp;
    }
  }
  ch.use_stream = use_stream; ch.cfg = best; ch.cost_splits = best_splits; ch.sshape = sshape;
  if (use_stream) {
    // the kernel the launch picks, its tile shape and the slabs it writes
    const bool exact = M % 96 == 0 && N % 96 == 0;
    const bool staged = vec && (sshape != 0 || !getenv("PDN_GEMM_STREAM_DIRECT"));   // (a shape other than 3 x 3 is set for aligned operands only)
    ch.kind = !staged ? (exact ? kStreamDirect : kStreamDirectEdge)
              : (sshape != 0 || !exact) ? kStreamLdsEdge : (getenv("PDN_GEMM_STREAM_NODMA") ? kStreamLds : kStreamDma);
  } else {
    const TileCfg& cfg = kCfgs[best];
    const int BM = cfg.waves_m * cfg.wm * 32, BN = cfg.waves_n * cfg.wn * 32;
    ch.tiles_m = (int)gemm_cdiv(M, BM);
    ch.tiles_n = (int)gemm_cdiv(N, BN);
    const int ktiles = (int)gemm_cdiv(K > 0 ? K : 1, cfg.bk);
    ch.k_per_split = (int)gemm_cdiv(ktiles, best_splits) * cfg.bk;
    ch.splits = (int)gemm_cdiv(K > 0 ? K : 1, ch.k_per_split);
    if (ch.splits < 1) ch.splits = 1;
  }
  return ch;
}

// the line PDN_GEMM_DEBUG prints for a streamed or tiled product (tools/gemm_fc_sweep.py and tests/test_gemm_variants.py parse it)
static inline int gemm_route_line(char* buf, size_t size, int M, int N, int K, int nbatch, const GemmLayout& lay,
                                  const GemmChoice& ch) {
  if (ch.use_stream)
    return snprintf(buf, size, "pdn_gemm_f32 M=%d N=%d K=%d nb=%d akin=%d bkin=%d vec=%d -> stream cfg=%d splits=%d sshape=%d kind=%s\n",
                    M, N, K, nbatch, (int)lay.a_kin, (int)lay.b_kin, (int)lay.vec, ch.cfg, ch.splits, ch.sshape,
                    kStreamKindNames[ch.kind]);
  return snprintf(buf, size, "pdn_gemm_f32 M=%d N=%d K=%d nb=%d akin=%d bkin=%d vec=%d -> tiled cfg=%d splits=%d\n", M, N, K, nbatch,
                  (int)lay.a_kin, (int)lay.b_kin, (int)lay.vec, ch.cfg, ch.cost_splits);
}
