// Stand-alone host check of pydynet_amd/csrc/weight_images_index.h, the header from which the batched weight-image builder
// (csrc/weight_images.hip) takes its job table, its arena layout and its keys.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_weight_images_check_cpu.py.  For sets that mix all five forms -- at the shapes of
// tests/test_weight_images_gpu.py, at the benchmark's two layer shapes (six layers, forward and backward forms) and for a
// set of more than PDNW_MAX_DESCS descriptors (several launches) -- it walks every workgroup and thread of every launch:
//   * every (descriptor, tile) and every (descriptor, piece, unit), and every column exponent, is written exactly once, the
//     first and the last workgroup of a descriptor belong to it, and no workgroup lies outside the table;
//   * what a workgroup writes lies inside its descriptor's image, the images are disjoint, PDNW_ALIGN-aligned and inside
//     pdnw_offset(descs, n) = pdnw_set_bytes;
//   * what it reads lies inside the weight (maxima over ALL pieces of its columns, then its own pieces);
//   * the constructors' fillers give the key the product's own launch forms from what its entry hands on.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../pydynet_amd/csrc/weight_images_index.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

// floats of the weight behind a descriptor, from its lowest block
static int64_t weight_floats(const PdnwDesc& d) {
  if (d.family == PDNW_RTS) {
    if (d.kind == 2) return (int64_t)(32 * d.n - 1) * d.ldb + RTS_K;
    if (d.kind == 1) return (int64_t)(d.g_off > d.u_off ? d.g_off : d.u_off) + (int64_t)(RTS_K - 1) * d.ldb + 16 * d.n;
    const int nb = 32 * d.n / d.nper;
    return (int64_t)(nb - 1) * d.bstride + (int64_t)(RTS_K - 1) * d.ldb + d.nper;
  }
  if (d.family == PDNW_ORS_NN) return (int64_t)(d.n * ORS_KP - 1) * d.ldb + ORS_N;
  const int nb = d.n / d.nper;
  return (int64_t)(nb - 1) * d.bstride + (int64_t)(ORS_N - 1) * d.ldb + (int64_t)d.nper * ORS_KP;
}

static void walk_set(const char* name, const std::vector<PdnwDesc>& ds) {
  const int n = (int)ds.size();
  const int64_t total = pdnw_offset(ds.data(), n);
  std::vector<unsigned char> arena((size_t)total, 0);           // a write count per byte
  std::vector<std::vector<int>> seen(n);                        // rts: per tile; ors: per (piece, unit), then 288 exponents
  for (int i = 0; i < n; ++i) {
    CHECK(pdnw_desc_ok(ds[i]), "%s: descriptor %d refused", name, i);
    seen[i].assign(ds[i].family == PDNW_RTS ? ds[i].n : ds[i].n * ORS_N * 4 + ORS_N, 0);
    const int64_t o = pdnw_offset(ds.data(), i);
    CHECK(o % PDNW_ALIGN == 0 && o + pdnw_image_bytes(ds[i]) <= total, "%s: image %d at %lld of %lld", name, i, (long long)o, (long long)total);
    if (i + 1 < n) CHECK(o + pdnw_image_bytes(ds[i]) <= pdnw_offset(ds.data(), i + 1), "%s: images %d and %d overlap", name, i, i + 1);
  }
  int launches = 0;
  for (int first = 0; first < n; first += PDNW_MAX_DESCS, ++launches) {
    PdnwTable t;
    memset(&t, 0, sizeof(t));
    const int count = n - first < PDNW_MAX_DESCS ? n - first : PDNW_MAX_DESCS;
    pdnw_table(ds.data(), first, count, &t);
    int expect_wgs = 0;
    for (int j = 0; j < count; ++j) {
      CHECK(t.job[j].wg0 == expect_wgs, "%s: job %d begins at %d, not %d", name, j, t.job[j].wg0, expect_wgs);
      CHECK(t.job[j].dst == pdnw_offset(ds.data(), first + j), "%s: job %d destination", name, j);
      CHECK(pdnw_job_of(t, t.job[j].wg0) == j, "%s: first workgroup of job %d", name, j);
      expect_wgs += pdnw_wgs(ds[first + j]);
      CHECK(pdnw_job_of(t, expect_wgs - 1) == j, "%s: last workgroup of job %d", name, j);
    }
    CHECK(t.nwgs == expect_wgs && t.njobs == count, "%s: %d workgroups, not %d", name, t.nwgs, expect_wgs);
    for (int wg = 0; wg < t.nwgs; ++wg) {
      const int j = pdnw_job_of(t, wg);
      CHECK(j >= 0 && j < count, "%s: workgroup %d outside the table", name, wg);
      const PdnwJob& q = t.job[j];
      const PdnwDesc& d = ds[first + j];
      const int l = wg - q.wg0, di = first + j;
      const int64_t wf = weight_floats(d), bytes = pdnw_image_bytes(d);
      auto put = [&](int64_t off, int len) {
        CHECK(off >= 0 && off + len <= bytes, "%s: descriptor %d writes %lld + %d of %lld", name, di, (long long)off, len, (long long)bytes);
        if (off >= 0 && off + len <= bytes)
          for (int b = 0; b < len; ++b) ++arena[(size_t)(q.dst + off + b)];
      };
      auto rd = [&](int64_t off, int len) { CHECK(off >= 0 && off + len <= wf, "%s: descriptor %d reads %lld + %d of %lld", name, di, (long long)off, len, (long long)wf); };
      if (q.family == PDNW_RTS) {
        CHECK(l >= 0 && l < d.n, "%s: tile %d of %d", name, l, d.n);
        ++seen[di][l];
        const int64_t img = (int64_t)l * RTS_TILE;
        for (int c = 0; c < 32; ++c)
          for (int k = 0; k < RTS_K; ++k)
            rd(q.kind == 2 ? rts_w_src_t(l, c, k, q.ldb) : rts_w_src(q.kind, l, c, k, q.nper, q.ldb, q.bstride, q.g_off, q.u_off), 1);
        for (int c = 0; c < 32; ++c)
          for (int ku = 0; ku < 36; ++ku) {
            CHECK(rts_img_unit(c, ku) + 16 <= RTS_PLANE, "unit");
            put(img + rts_img_unit(c, ku), 16);
            put(img + RTS_PLANE + rts_img_unit(c, ku), 16);
          }
        put(img + RTS_TAIL, 256);
        continue;
      }
      const int y = pdnw_ors_colrange(l), chunk = pdnw_ors_chunk(l);
      CHECK(y >= 0 && y < PDNW_ORS_COLS && chunk >= 0 && chunk < pdnw_ors_chunks(d.n), "%s: local workgroup %d", name, l);
      for (int tid = 0; tid < 256; ++tid) {
        const int i = pdnw_ors_unit(y, tid);
        const bool on = i < ORS_N * 4;
        const int dcol = on ? i >> 2 : ORS_N - 1, u = i & 3;
        CHECK(dcol >= pdnw_ors_col0(y) && dcol < pdnw_ors_col0(y) + 64, "%s: column %d of range %d", name, dcol, y);
        // the maxima: every piece of the thread's column (NT), or the range's columns by float4 and row group (NN)
        if (q.family == PDNW_ORS_NT) {
          for (int s = 0; s < d.n; ++s) rd(ors_w_src_nt(s, dcol, u, q.nper, q.ldb, q.bstride), 8);
        } else if (4 * pdnw_nn_max_c4(tid) < pdnw_ors_ncols(y)) {
          for (int k = pdnw_nn_max_row(tid); k < d.n * ORS_KP; k += 16) {
            const int64_t src = ors_w_src_nn(k / ORS_KP, (k % ORS_KP) * 72 + 16 * y + pdnw_nn_max_c4(tid), q.ldb);
            CHECK(src == (int64_t)k * q.ldb + 64 * y + 4 * pdnw_nn_max_c4(tid), "%s: NN maximum source", name);
            rd(src, 4);
          }
        }
        if (chunk == 0 && u == 0 && on) { ++seen[di][d.n * ORS_N * 4 + dcol]; put(pdnw_exp_offset(d) + 4 * dcol, 4); }
        for (int s = pdnw_ors_piece0(chunk); s < pdnw_ors_piece1(chunk, d.n); ++s) {
          if (q.family == PDNW_ORS_NT) rd(ors_w_src_nt(s, dcol, u, q.nper, q.ldb, q.bstride), 8);
          else {
            // staged by the workgroup: float4 16 y .. of the piece's 32 rows; the thread's eight values lie inside them
            const int nc4 = pdnw_ors_ncols(y) / 4;
            CHECK(dcol / 4 >= 16 * y && dcol / 4 < 16 * y + nc4, "%s: column %d not staged", name, dcol);
            for (int e = tid; e < ORS_KP * nc4; e += 256) rd(ors_w_src_nn(s, (e / nc4) * 72 + 16 * y + e % nc4, q.ldb), 4);
          }
          if (!on) continue;
          ++seen[di][(s * ORS_N + dcol) * 4 + u];
          CHECK(ors_img_unit(dcol, u) + 16 <= ORS_PLANE, "unit");
          put((int64_t)s * ORS_PIECE + ors_img_unit(dcol, u), 16);
          put((int64_t)s * ORS_PIECE + ORS_PLANE + ors_img_unit(dcol, u), 16);
        }
      }
    }
  }
  int64_t units = 0;
  for (int i = 0; i < n; ++i)
    for (size_t e = 0; e < seen[i].size(); ++e) { CHECK(seen[i][e] == 1, "%s: descriptor %d element %zu written %d times", name, i, e, seen[i][e]); ++units; }
  // every byte of every image written exactly once, nothing between the images
  for (int i = 0; i < n; ++i) {
    const int64_t o = pdnw_offset(ds.data(), i), b = pdnw_image_bytes(ds[i]);
    for (int64_t x = 0; x < b; ++x) CHECK(arena[(size_t)(o + x)] == 1, "%s: image %d byte %lld written %d times", name, i, (long long)x, arena[(size_t)(o + x)]);
    for (int64_t x = o + b; x < pdnw_offset(ds.data(), i + 1); ++x) CHECK(arena[(size_t)x] == 0, "%s: padding behind image %d written", name, i);
  }
  printf("%s: %d descriptors, %d launch(es), %lld bytes, %lld tiles / units / exponents: every one written once\n", name, n, launches,
         (long long)total, (long long)units);
}

// the keys: constructor fillers against what the product entries hand their launch (csrc/gemm_rowres.hip: rowres_launch
// fills RowTileArgs with B, N, nblocks, ldb, b_block_stride, and the epilogue's g_off / u_off / F)
static void check_fillers(const float* base) {
  const int K = 288;
  for (int D : {96, 288}) {
    const int64_t stride = (int64_t)K * D + 64;
    // pdn_qkv_rope_*: rowres_launch(x, wq, ..., N = 3 D, K, ldx, ldb = D, ldc, 0, nblocks = 3, w_stride), epilogue 3
    CHECK(pdnw_same(pdnw_desc_of_qkv(base, stride, D), pdnw_key_rts(3, base, 3 * D, 3, D, stride, 0, 0, 0)), "qkv key D=%d", D);
  }
  for (int F : {32, 768})
    for (int sign : {1, -1}) {
      const int64_t ws = (int64_t)K * F + 128, w_stride = sign * ws;
      const float* w_gate = base + (sign < 0 ? ws : 0);
      // pdn_gateup_swiglu_*: wbase = the lower matrix, g_off / u_off = where gate / up begin, nblocks = 2, stride |w_stride|
      const float* wbase = w_stride < 0 ? w_gate + w_stride : w_gate;
      CHECK(pdnw_same(pdnw_desc_of_gateup(w_gate, w_stride, F),
                      pdnw_key_rts(1, wbase, 2 * F, 2, F, ws, w_stride < 0 ? (unsigned)ws : 0u, w_stride < 0 ? 0u : (unsigned)ws, F)),
            "gate | up key F=%d sign=%d", F, sign);
      CHECK(pdnw_desc_of_gateup(w_gate, w_stride, F).B == base, "gate | up base");
      // pdn_swiglu_bwd_gemm_f32: rowres_launch(dy, w_down, ..., N = F, K, ldy, ldb = K, 2 F, 1, nblocks = 1, 0), epilogue 2
      CHECK(pdnw_same(pdnw_desc_of_down_t(base, F, K), pdnw_key_rts(2, base, F, 1, K, 0, 0, 0, F)), "down^T key F=%d", F);
    }
  // a key differs as soon as one field does
  PdnwDesc a = pdnw_key_ors(base, 864, 288, 1, 288, 288 * 288), b = a;
  CHECK(pdnw_same(a, b), "equal keys");
  b.ldb = 292; CHECK(!pdnw_same(a, b), "ldb"); b = a;
  b.B = base + 4; CHECK(!pdnw_same(a, b), "B"); b = a;
  b.family = PDNW_ORS_NN; CHECK(!pdnw_same(a, b), "family"); b = a;
  b.nper = 27; CHECK(!pdnw_same(a, b), "nper");
  CHECK(!pdnw_same(pdnw_key_ors(base, 288, 288, 0, 0, 0), pdnw_key_ors(base, 288, 288, 1, 0, 0)), "NN / NT");
  printf("fillers: the constructors' keys equal the products'\n");
}

int main() {
  static std::vector<float> weights(1 << 20);   // (addresses only: nothing is dereferenced)
  const float* w = weights.data();
  check_fillers(w);
  const int K = 288;
  // the shapes of tests/test_weight_images_gpu.py: F = 32, 3 x 288 columns, K = 288 NN / NT, K = 768 NN, 3 x 288 NT blocks, and
  // a weight with ldb larger than its width
  std::vector<PdnwDesc> small = {
      pdnw_desc_of_qkv(w, (int64_t)K * 288, 288), pdnw_desc_of_gateup(w, (int64_t)K * 32, 32), pdnw_desc_of_gateup(w + K * 32, -(int64_t)K * 32, 32),
      pdnw_desc_of_down_t(w, 32, K),              pdnw_key_ors(w, 288, 288, 0, 0, 0),           pdnw_key_ors(w, 288, 288, 1, 0, 0),
      pdnw_key_ors(w, 768, 288, 0, 0, 0),         pdnw_key_ors(w, 864, 288, 1, 288, 288 * 288), pdnw_key_ors(w, 288, 320, 0, 0, 0),
      pdnw_key_ors(w, 288, 320, 1, 0, 0)};
  walk_set("test shapes", small);
  // the benchmark: embed 288, ffn 768, six layers
  std::vector<PdnwDesc> fwd, bwd;
  for (int layer = 0; layer < 6; ++layer) {
    fwd.push_back(pdnw_desc_of_qkv(w, (int64_t)K * 288, 288));
    fwd.push_back(pdnw_key_ors(w, 288, 288, 0, 0, 0));
    fwd.push_back(pdnw_desc_of_gateup(w, (int64_t)K * 768, 768));
    fwd.push_back(pdnw_key_ors(w, 768, 288, 0, 0, 0));
    bwd.push_back(pdnw_key_ors(w, 864, 288, 1, 288, 288 * 288));
    bwd.push_back(pdnw_key_ors(w, 288, 288, 1, 0, 0));
    bwd.push_back(pdnw_desc_of_down_t(w, 768, K));
    bwd.push_back(pdnw_key_ors(w, 1536, 768, 1, 768, 288 * 768));
  }
  walk_set("benchmark forward", fwd);
  walk_set("benchmark backward", bwd);
  std::vector<PdnwDesc> many;
  for (int r = 0; r < 7; ++r) many.insert(many.end(), small.begin(), small.end());      // 70 > PDNW_MAX_DESCS: two launches
  walk_set("two launches", many);
  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("weight_images_check: all sets pass\n");
  return 0;
}
