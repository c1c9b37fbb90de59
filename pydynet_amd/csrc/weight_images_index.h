// Index arithmetic of the batched weight-image builder (csrc/weight_images.hip, include/pdn_wimages.h), shared by the kernel,
// the library's host side and a host checker (tests/weight_images_check.cpp): what a descriptor holds, where its image lies
// in a set's arena, and which (descriptor, unit, sub-range) a workgroup of the one launch builds.  Nothing here depends on
// HIP.
//
// A DESCRIPTOR names one (weight, form): the W-params a product fills for its own per-call pass, minus the destination.
//   family PDNW_RTS:    the tile images of csrc/rowtile_split.hip, kind 3 (q | k | v), 1 (gate | up), 2 (W_down along k);
//                       n = tiles, nper = columns per block.  One workgroup per tile (rts_w_kernel's body).
//   family PDNW_ORS_NN / PDNW_ORS_NT: the piece images of csrc/outres_split.hip and their 288 column exponents;
//                       n = pieces, nper = pieces per block.  The image is cut into PDNW_ORS_COLS column ranges of 64 columns
//                       (256 units of a piece, one per thread) and chunks of PDNW_ORS_CHUNK pieces: a workgroup first takes
//                       the maxima of its 64 columns over ALL pieces (a maximum does not depend on the order, so the
//                       exponents are those of the per-call pass), then writes its pieces' units.  The exponents are
//                       written by the workgroups of chunk 0.
// ARENA: image after image in descriptor order, each at a multiple of PDNW_ALIGN bytes (the products copy an image by
// 16-byte units, global -> registers or LDS-DMA); an ors image is followed by its 288 exponents.
#pragma once
#include <stdint.h>
#include "rowtile_split_index.h"
#include "outres_split_index.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDNW_HD __host__ __device__ __forceinline__
#else
#define PDNW_HD inline
#endif

#define PDNW_RTS 0
#define PDNW_ORS_NN 1
#define PDNW_ORS_NT 2
#define PDNW_ALIGN 256
#define PDNW_ORS_COLS 5                      // column ranges of 64 (the last: 32 columns)
#define PDNW_ORS_CHUNK 4                     // pieces per workgroup
#define PDNW_MAX_DESCS 48                    // descriptors per launch (the job table travels by value)

// 64 bytes; include/pdn_wimages.h hands it out as opaque records of pdnw_desc_bytes()
struct PdnwDesc {
  const float* B;
  int64_t ldb, bstride;
  int32_t family, kind;                      // kind: the rts kind (1, 2, 3); 0 for the ors families
  int32_t n, nper;
  uint32_t g_off, u_off;
  int64_t reserved[2];
};

// one entry of the job table: a descriptor, where its image begins in the arena, and its first workgroup
struct PdnwJob {
  const float* B;
  int64_t ldb, bstride, dst;
  int32_t family, kind, n, nper;
  uint32_t g_off, u_off;
  int32_t wg0, pad;
};
struct PdnwTable {
  int32_t njobs, nwgs;
  PdnwJob job[PDNW_MAX_DESCS];
};

PDNW_HD int64_t pdnw_round_up(int64_t v) { return (v + PDNW_ALIGN - 1) / PDNW_ALIGN * PDNW_ALIGN; }
PDNW_HD bool pdnw_desc_ok(const PdnwDesc& d) {
  if (d.B == nullptr || d.n < 1 || d.nper < 1) return false;
  if (d.family == PDNW_RTS) return d.kind >= 1 && d.kind <= 3;
  return (d.family == PDNW_ORS_NN || d.family == PDNW_ORS_NT) && d.kind == 0 && d.n <= ORS_MAX_K / ORS_KP;
}
// bytes of a descriptor's image (ors: with its exponents), before rounding
PDNW_HD int64_t pdnw_image_bytes(const PdnwDesc& d) {
  return d.family == PDNW_RTS ? (int64_t)d.n * RTS_TILE : (int64_t)d.n * ORS_PIECE + ORS_N * 4;
}
PDNW_HD int64_t pdnw_exp_offset(const PdnwDesc& d) { return (int64_t)d.n * ORS_PIECE; }   // the ors exponents, from the image
PDNW_HD int pdnw_ors_chunks(int n) { return (n + PDNW_ORS_CHUNK - 1) / PDNW_ORS_CHUNK; }
PDNW_HD int pdnw_wgs(const PdnwDesc& d) { return d.family == PDNW_RTS ? d.n : pdnw_ors_chunks(d.n) * PDNW_ORS_COLS; }
// arena offset of descriptor i of a set (i == n: the set's size)
PDNW_HD int64_t pdnw_offset(const PdnwDesc* d, int i) {
  int64_t o = 0;
  for (int j = 0; j < i; ++j) o += pdnw_round_up(pdnw_image_bytes(d[j]));
  return o;
}
// the job table of descriptors first .. first + count - 1 of a set (count <= PDNW_MAX_DESCS)
PDNW_HD void pdnw_table(const PdnwDesc* d, int first, int count, PdnwTable* t) {
  int64_t o = pdnw_offset(d, first);
  int wg = 0;
  t->njobs = count;
  for (int j = 0; j < count; ++j) {
    const PdnwDesc& s = d[first + j];
    PdnwJob& q = t->job[j];
    q.B = s.B; q.ldb = s.ldb; q.bstride = s.bstride; q.dst = o; q.family = s.family; q.kind = s.kind; q.n = s.n; q.nper = s.nper;
    q.g_off = s.g_off; q.u_off = s.u_off; q.wg0 = wg; q.pad = 0;
    o += pdnw_round_up(pdnw_image_bytes(s));
    wg += pdnw_wgs(s);
  }
  t->nwgs = wg;
}
// workgroup `wg` of the launch: its job, and its index inside the job
PDNW_HD int pdnw_job_of(const PdnwTable& t, int wg) {
  int j = 0;
  while (j + 1 < t.njobs && wg >= t.job[j + 1].wg0) ++j;
  return j;
}
// ors: local workgroup l = chunk * PDNW_ORS_COLS + column range
PDNW_HD int pdnw_ors_chunk(int l) { return l / PDNW_ORS_COLS; }
PDNW_HD int pdnw_ors_colrange(int l) { return l % PDNW_ORS_COLS; }
PDNW_HD int pdnw_ors_piece0(int chunk) { return chunk * PDNW_ORS_CHUNK; }
PDNW_HD int pdnw_ors_piece1(int chunk, int n) { return ors_min_i(n, (chunk + 1) * PDNW_ORS_CHUNK); }
// thread `tid` of column range y owns unit i = 256 y + tid of every piece (i < 1152): column i >> 2, unit i & 3 -- the
// thread mapping of ors_w_img_kernel, whose grid.y is the column range
PDNW_HD int pdnw_ors_unit(int y, int tid) { return y * 256 + tid; }
PDNW_HD int pdnw_ors_col0(int y) { return 64 * y; }
PDNW_HD int pdnw_ors_ncols(int y) { return ors_min_i(64, ORS_N - 64 * y); }
// NN maxima: thread tid reads float4 (tid & 15) of its range's 64 columns in the rows tid >> 4, + 16, ... of B
PDNW_HD int pdnw_nn_max_c4(int tid) { return tid & 15; }
PDNW_HD int pdnw_nn_max_row(int tid) { return tid >> 4; }

// ---- the fillers' keys: what a product's W-params must equal for a descriptor to serve it ---------------------------------
PDNW_HD bool pdnw_same(const PdnwDesc& a, const PdnwDesc& b) {
  return a.B == b.B && a.ldb == b.ldb && a.bstride == b.bstride && a.family == b.family && a.kind == b.kind && a.n == b.n &&
         a.nper == b.nper && a.g_off == b.g_off && a.u_off == b.u_off;
}
// q | k | v, gate | up, W_down along k: from the arguments of pdn_rowtile_split_launch (RowTileArgs: epi, B, N, nblocks, ldb,
// b_block_stride, g_off, u_off, F)
PDNW_HD PdnwDesc pdnw_key_rts(int epi, const float* B, int N, int nblocks, int64_t ldb, int64_t b_block_stride, unsigned g_off,
                              unsigned u_off, int F) {
  PdnwDesc d = {};
  d.B = B; d.family = PDNW_RTS; d.kind = epi; d.n = epi == 1 ? F / 16 : N / 32; d.nper = N / nblocks; d.ldb = ldb;
  d.bstride = nblocks > 1 ? b_block_stride : 0; d.g_off = g_off; d.u_off = u_off;
  return d;
}
// the descriptor constructors of include/pdn_wimages.h, from the arguments of the products' ENTRIES; what those entries hand
// pdn_rowtile_split_launch (csrc/gemm_rowres.hip) must give the same key, which tests/weight_images_check.cpp holds
PDNW_HD PdnwDesc pdnw_desc_of_qkv(const float* wq, int64_t w_stride, int D) { return pdnw_key_rts(3, wq, 3 * D, 3, D, w_stride, 0, 0, 0); }
PDNW_HD PdnwDesc pdnw_desc_of_gateup(const float* w_gate, int64_t w_stride, int F) {
  // (the lower matrix is the base, the other lies ws floats above it)
  const int64_t ws = w_stride < 0 ? -w_stride : w_stride;
  return pdnw_key_rts(1, w_stride < 0 ? w_gate + w_stride : w_gate, 2 * F, 2, F, ws, w_stride < 0 ? (unsigned)ws : 0u,
                      w_stride < 0 ? 0u : (unsigned)ws, F);
}
PDNW_HD PdnwDesc pdnw_desc_of_down_t(const float* w_down, int F, int K) { return pdnw_key_rts(2, w_down, F, 1, K, 0, 0, 0, F); }
// the output-resident products: from the arguments of ors_launch (B, K, ldb, b_trans, kb, b_bstride)
PDNW_HD PdnwDesc pdnw_key_ors(const float* B, int K, int64_t ldb, int b_trans, int kb, int64_t b_bstride) {
  PdnwDesc d = {};
  const int np = K / ORS_KP;
  d.B = B; d.family = b_trans ? PDNW_ORS_NT : PDNW_ORS_NN; d.kind = 0; d.n = np; d.nper = kb > 0 ? kb / ORS_KP : np; d.ldb = ldb;
  d.bstride = kb > 0 ? b_bstride : 0;
  return d;
}
