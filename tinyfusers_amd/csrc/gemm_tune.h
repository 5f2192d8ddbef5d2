// Which (tile, split-K, family, tile order) a launch gets: the cost model and the untuned defaults, the tuning table with its C entries, and the
// per-shape autotuner.  Host side only (included by gemm.hip).
#pragma once
#include "gemm_family.h"
#include <stdlib.h>
#include <array>
#include <map>

// Cost model (microseconds) calibrated on MI355X with tools/gemm_bench.py: a K tile costs the larger of its LDS-DMA
// ingest time ((bm+bn)*128 B at ~90 GB/s per CU) and its MFMA time (~7 TFLOP/s per CU sustained), one block per CU per
// wave of blocks; split-K adds a reduce launch and an fp32 round trip of the output.
static TileCfg choose_tiles(int M, int N, int K, int act, bool allow_split) {
  static const int cand[][2] = {{128, 160}, {64, 160}, {128, 128}, {64, 128}, {128, 64}, {64, 64}};
  const int ncand = 6;
  int ktiles = (K + 63) / 64;
  TileCfg best = {64, 64, 1};
  double best_t = 1e30;
  for (int ci = 0; ci < ncand; ++ci) {
    int bm = cand[ci][0], bn = cand[ci][1];
    if (act == 1 && (bn % 64) != 0) continue;           // GEGLU pairs 16-row blocks inside a wave tile
    int ntm = (M + bm - 1) / bm, ntn = (N + bn - 1) / bn;
    double tiles = (double)ntm * ntn;
    double t_ing = (bm + bn) * 128.0 / 90e3, t_mfma = (double)bm * bn * 128.0 / 7.0e6;
    double t_tile = (t_ing > t_mfma ? t_ing : t_mfma) + 0.05;
    int max_split = (allow_split && act == 0) ? 32 : 1;
    for (int sk = 1; sk <= max_split; sk *= 2) {
      if (sk > 1 && ktiles / sk < 8) break;
      double blocks = tiles * sk;
      double waves = ceil(blocks / 256.0);
      double t = 3.0 + waves * ((ktiles + sk - 1) / sk) * t_tile;
      if (sk > 1) t += 4.0 + (double)M * N * 4.0 * (sk + 1) / 3.0e6;
      if (t < best_t) { best_t = t; best = {bm, bn, sk}; }
    }
  }
  return best;
}

struct TunedCfg { TileCfg c; int variant; int order; };   // variant: a Variant (gemm_family.h)

// untuned default for a launch that carries the input GroupNorm: the first admissible (tile, variant), split-K of the cost model
static TunedCfg gi_default(const GemmP& p) {
  static const int cand[][2] = {{64, 160}, {128, 160}, {64, 128}, {128, 128}, {64, 64}, {128, 64}};
  TileCfg m = choose_tiles(p.M, p.N, p.K, p.act, true);
  for (int ci = 0; ci < 6; ++ci)
    for (int v = (p.S == 3 ? V_PATCH : V_RING); v <= V_ALL8; ++v)
      if (gi_tile_ok(p, cand[ci][0], cand[ci][1], v)) {
        int sk = m.splitk;
        long long blocks = (long long)((p.M + cand[ci][0] - 1) / cand[ci][0]) * ((p.N + cand[ci][1] - 1) / cand[ci][1]);
        while (sk > 1 && (blocks * sk > 1024 || p.ktiles / sk < 4)) sk >>= 1;
        return {{cand[ci][0], cand[ci][1], sk}, v, 0};
      }
  return {m, V_RING, 0};
}

// block-scaled e4m3 launches: which (tile, split) of the ping-pong kernel a launch gets without a table row; tile.bm = 0 when none can take it
static TunedCfg mx_default(const GemmP& p) {
  static const int cand[][2] = {{192, 160}, {192, 128}, {256, 128}, {256, 160}};
  TunedCfg best = {{0, 0, 1}, V_PP, 0};
  // the patch form where it applies: 2.0-2.4 against 1.2-1.45 PFLOP/s on config 5's 3x3 convs (tools/mx_bench.py)
  if (pp3_setup(p, 192, 128) && (long long)(p.M / 192) * ((p.N + 127) / 128) >= 128) return {{192, 128, 1}, V_PP3, 1};
  long long best_waste = -1;
  for (int ci = 0; ci < 4; ++ci) {
    const int bm = cand[ci][0], bn = cand[ci][1];
    if (!pp_ok(p, bn, bm)) continue;
    if (bn == 160 && p.N % 160 != 0 && p.N % 128 == 0) continue;
    const long long waste = (long long)((p.M + bm - 1) / bm) * bm * (long long)((p.N + bn - 1) / bn) * bn - (long long)p.M * p.N;
    if (best_waste < 0 || waste < best_waste) { best_waste = waste; best = {{bm, bn, 1}, V_PP, 0}; }
  }
  return best;
}

// ---- the tuning table: one (tile, split-K, family, order) per shape key, loaded from a file (the shipped gemm_tune_gfx950.txt) or filled by the tuner
static int g_autotune = 1;     // 0: cost model only; 1: a shape missing from the table is tuned on its first eager use; 2: table only -- a missing shape is an error (every rank of a multi-GPU run must pick the same kernels)
typedef std::array<int, 10> TuneKey;                      // {M, N, K, C1, C2, S, stride, upsample, act, flags}
static std::map<TuneKey, TunedCfg> g_tuned;
static bool g_trace_keys = false;                       // tf_gemm_tune_trace: remember every shape key a launch looks up (tools/gemm_keys.py)
static std::map<TuneKey, bool> g_traced;
static TuneKey tune_key(const GemmP& p) {
  return {p.M, p.N, p.K, p.C1, p.C2, p.S, p.stride, p.ups, p.act,
          (p.bias ? 1 : 0) | (p.residual ? 2 : 0) | (p.bias_nc ? 4 : 0) | (p.ln_colsum ? 8 : 0) | (p.gi_part ? 16 : 0) | (p.fp8 ? 64 : 0) | (p.out8 ? 128 : 0) | (p.out32 ? 256 : 0) | (p.mx ? 512 : 0) | (p.bf16 ? 1024 : 0)};   // (on_z shares the plain key: same tile, another reduce kernel)
}
static void tune_cfg_out(const TunedCfg& t, int* cfg) { cfg[0] = t.c.bm; cfg[1] = t.c.bn; cfg[2] = t.c.splitk; cfg[3] = t.variant; cfg[4] = t.order; }

extern "C" {
int tf_gemm_autotune(int mode) {
  TF_REQUIRE(mode >= 0 && mode <= 2, "tf_gemm_autotune: mode=%d (0 cost model only, 1 tune missing shapes on first use, 2 table only: a missing shape is an error)", mode);
  g_autotune = mode;
  if (!mode) g_tuned.clear();
  return TF_OK;
}
// host-side view of the table (no device work): what the launch of a shape would pick.  key = {M, N, K, C1, C2, S, stride, upsample, act, flags}
// as tf_gemm_tune_save writes them, cfg = {bm, bn, splitk, variant, order}; TF_E_STATE when the shape has no row
int tf_gemm_tune_query(const int* key, int* cfg) {
  TF_REQUIRE(key && cfg, "tf_gemm_tune_query: null argument");
  TuneKey k;
  for (int i = 0; i < 10; ++i) k[i] = key[i];
  auto it = g_tuned.find(k);
  if (it == g_tuned.end()) { tf_set_error("tf_gemm_tune_query: shape M=%d N=%d K=%d has no row", key[0], key[1], key[2]); return TF_E_STATE; }
  tune_cfg_out(it->second, cfg);
  return TF_OK;
}
// which shapes does a workload consult?  tf_gemm_tune_trace(1) starts remembering every key a launch looks up (and whether it had a row),
// tf_gemm_tune_trace_dump writes them, one per line: the ten key fields and 1 / 0 (tools/gemm_keys.py -> tests/golden/gemm_keys.json)
int tf_gemm_tune_trace(int on) { g_trace_keys = on != 0; if (on) g_traced.clear(); return TF_OK; }
int tf_gemm_tune_trace_dump(const char* path) {
  TF_REQUIRE(path, "tf_gemm_tune_trace_dump: null path");
  FILE* f = fopen(path, "w");
  TF_REQUIRE(f, "tf_gemm_tune_trace_dump: cannot open %s", path);
  for (auto& kv : g_traced) {
    for (int i = 0; i < 10; ++i) fprintf(f, "%d ", kv.first[i]);
    fprintf(f, "%d\n", kv.second ? 1 : 0);
  }
  fclose(f);
  return TF_OK;
}
int tf_gemm_tune_count(int* n) { TF_REQUIRE(n, "tf_gemm_tune_count: null argument"); *n = (int)g_tuned.size(); return TF_OK; }
int tf_gemm_tune_entry(int index, int* key, int* cfg) {
  TF_REQUIRE(key && cfg && index >= 0 && index < (int)g_tuned.size(), "tf_gemm_tune_entry: index %d out of range", index);
  auto it = g_tuned.begin();
  std::advance(it, index);
  for (int i = 0; i < 10; ++i) key[i] = it->first[i];
  tune_cfg_out(it->second, cfg);
  return TF_OK;
}
// persist / restore the tuner's choices (one line per shape) so that profiled or repeated runs skip the tuning launches
int tf_gemm_tune_save(const char* path) {
  TF_REQUIRE(path, "tf_gemm_tune_save: null path");
  FILE* f = fopen(path, "w");
  TF_REQUIRE(f, "tf_gemm_tune_save: cannot open %s", path);
  for (auto& kv : g_tuned) {
    for (int i = 0; i < 10; ++i) fprintf(f, "%d ", kv.first[i]);
    fprintf(f, "%d %d %d %d %d\n", kv.second.c.bm, kv.second.c.bn, kv.second.c.splitk, kv.second.variant, kv.second.order);
  }
  fclose(f);
  return TF_OK;
}
// The rows of a file are input from outside the program, and a key holds fewer fields than a launch: what is accepted here is the table's own
// rule (per family: the tiles and splits a row may name), not the families' admits() -- a row a launch then cannot take is resolved in run_gemm.
int tf_gemm_tune_load(const char* path) {
  TF_REQUIRE(path, "tf_gemm_tune_load: null path");
  FILE* f = fopen(path, "r");
  if (!f) return TF_OK;                                  // no cache yet: tune on first use
  TuneKey k; int bm, bn, sk, variant, order;
  for (;;) {
    int n = 0;
    for (int i = 0; i < 10; ++i) n += fscanf(f, "%d", &k[i]);
    n += fscanf(f, "%d %d %d %d %d", &bm, &bn, &sk, &variant, &order);
    if (n != 15) break;
    const bool f8 = (k[9] & 64) != 0;
    bool ok = (bm == 64 || bm == 128 || (f8 && bm == 256 && bn == 64) || (!f8 && bm == 256 && bn == 128) || variant == V_PP) && (bn == 64 || bn == 128 || (!f8 && bn == 160) || variant == V_PP) &&
              sk >= 1 && sk <= 32;
    if (((f8 && variant != V_PP) || (bm == 256 && variant != V_PP && variant != V_C8)) && variant != V_RING) ok = false;
    if (variant == V_PP) ok = ((bm == 256 && (bn == 128 || bn == 160 || (!f8 && bn == 256))) || (bm == 192 && (bn == 128 || bn == 160))) && sk >= 1 && sk <= 32;
    // rows the tuner itself never emits: GEGLU (act = 1) pairs 16-row value|gate blocks inside a wave tile (bn % 64 == 0), and
    // neither GEGLU nor the LayerNorm fold (flag bit 8) can be split along K
    const int act = k[8], ln = k[9] & 8;
    if (act == 1 && (bn % 64) != 0) ok = false;
    if ((act == 1 || ln || (k[9] & 256)) && sk > 1) ok = false;
    if (variant == V_C4) ok = bm == 128 && bn == 128 && sk == 1 && !f8;
    if (variant == V_C8) ok = bm == 256 && bn == 128 && sk == 1 && !f8;
    if (variant == V_AR) ok = bm == 128 && bn == 128 && sk == 1 && !f8;
    if (variant == V_PP3) ok = bm == 192 && (bn == 128 || bn == 160) && sk == 1 && k[5] == 3 && k[6] == 1 && act == 0 && !ln && (!f8 || (k[9] & 512));   // the patch form: 3x3 / stride 1; e4m3 only block-scaled
    if (ok) g_tuned[k] = {{bm, bn, sk}, variant < V_RING || variant >= V_COUNT ? V_RING : variant, order != 0 ? 1 : 0};
  }
  fclose(f);
  return TF_OK;
}
}  // extern "C"

// ---- per-shape autotuner ("measure, don't guess"): the first eager call of a shape times every admissible
// (tile, split-K, family, tile order) on the caller's own buffers with HIP events and caches the winner.  Never runs
// inside a stream capture (a captured shape that was never seen eagerly falls back to the cost model).
#define TF_SPLITK_WS_CAP ((size_t)64 << 20)
#define TF_FLUSH_BYTES ((size_t)384 << 20)
static void* g_flush = nullptr;
// One configuration, timed.  In the real step every layer's weights come from HBM (1.7 GB of weights per step never stay cached), so each
// timed launch is preceded by a cache flush (a 384 MiB memset, outside the timed interval): median of 5 behind a warm-up launch.
static int time_config(const GemmP& p, TileCfg c, int variant, int order, void* workspace, hipStream_t st, float* ms) {
  if (!g_flush) TF_HIP(hipMalloc(&g_flush, TF_FLUSH_BYTES));
  int rc = launch_one(p, c, variant, order, workspace, st);   // warm-up
  if (rc) return rc;
  hipEvent_t a, b;
  TF_HIP(hipEventCreate(&a)); TF_HIP(hipEventCreate(&b));
  float tv[5];
  for (int r = 0; r < 5; ++r) {
    TF_HIP(hipMemsetAsync(g_flush, r, TF_FLUSH_BYTES, st));
    TF_HIP(hipEventRecord(a, st));
    rc = launch_one(p, c, variant, order, workspace, st);
    if (rc) break;
    TF_HIP(hipEventRecord(b, st));
    TF_HIP(hipEventSynchronize(b));
    TF_HIP(hipEventElapsedTime(&tv[r], a, b));
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  if (rc) return rc;
  for (int i = 0; i < 5; ++i) for (int j = i + 1; j < 5; ++j) if (tv[j] < tv[i]) { float t = tv[i]; tv[i] = tv[j]; tv[j] = t; }
  *ms = tv[2];
  return TF_OK;
}

// What the tuner tries for a launch, in the order it tries it (the winner is the first strict minimum).  Whether a family can take a configuration
// is the family's own answer (family_admits); the rules written out here are the tuner's: which admissible configurations are worth a measurement.
struct Candidate { TileCfg c; int variant, order; bool drop_gn_stats; };   // drop_gn_stats: the tiling does not map onto whole images, so it is timed (and would run) without the statistics epilogue
static const int kTiles8[][2] = {{128, 128}, {64, 128}, {128, 64}, {256, 64}, {64, 64}};
static const int kNumTiles8 = 5;
static std::vector<Candidate> tune_candidates(const GemmP& p, void* workspace, size_t workspace_bytes) {
  std::vector<Candidate> out;
  auto add = [&](TileCfg c, int variant, int norders) {
    const bool drop = p.gn_part && c.splitk == 1 && !gn_tile_ok(p, stats_bm(c.bm, variant), c.bn);
    for (int order = 0; order < norders; ++order) out.push_back({c, variant, order, drop});
  };
  auto tiles = [&](int bm, int bn) { return (long long)((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn); };
  // may the K range be split sk ways at all?  (GEGLU, the LayerNorm fold and the raw fp32 output need the whole range in one block)
  auto can_split = [&](int sk, int variant) {
    return !(p.act == 1 || p.ln_colsum || p.out32 || ktiles_for(p, variant) / sk < 4 || !workspace || (size_t)sk * p.M * p.N * 4 > workspace_bytes);
  };
  // the k_igemm forms (k_igemm8's tiles for fixed-scale e4m3; block-scaled launches have the ping-pong kernel only: below)
  static const int cand[][2] = {{128, 160}, {64, 160}, {128, 128}, {64, 128}, {128, 64}, {64, 64}, {256, 128}};
  for (int ci = 0; ci < (p.mx ? 0 : p.fp8 ? kNumTiles8 : 7); ++ci) {
    int bm = p.fp8 ? kTiles8[ci][0] : cand[ci][0], bn = p.fp8 ? kTiles8[ci][1] : cand[ci][1];
    if (p.act == 1 && (bn % 64) != 0) continue;
    if (bm >= 128 && p.M <= 64) continue;
    if (bm == 256 && p.M <= 128) continue;
    // the 256x128 fp16 tile: plain deep ring, channel counts on the 64 grid, and only where it still leaves every CU a tile
    if (!p.fp8 && bm == 256 && (gemm_generic(p) || p.gi_part || p.ln_colsum || tiles(256, 128) < 256)) continue;
    if (bn >= 128 && p.N <= 64) continue;
    for (int sk = 1; sk <= 32; sk *= 2) {
      if (sk > 1 && !can_split(sk, V_RING)) break;
      long long blocks = tiles(bm, bn) * sk;
      if (sk > 1 && blocks > 1024) break;
      for (int v = V_RING; v <= V_ALL8; ++v) {
        if ((p.fp8 || bm == 256) && v != V_RING) continue;   // k_igemm8 and the 256-row tile have the deep ring only
        if (v == V_ALL8 && gemm_generic(p)) continue;       // (it would run the deep ring again)
        if (v == V_WIDE && (bm == 128 && bn == 160)) continue;
        if (v == V_WIDE && blocks <= 256) continue;          // two blocks per CU need more blocks than CUs
        if (v == V_PATCH && !patch_admits(p, bm, bn)) continue;   // (likewise)
        if (!family_admits(v, p, {bm, bn, sk})) continue;
        add({bm, bn, sk}, v, (p.M + bm - 1) / bm == 1 ? 1 : 2);   // a single m tile: both orders coincide
      }
    }
  }
  // the ping-pong kernel: {256, 192} x {160, 128, 256} tiles for launches that still give most CUs a tile with them
  static const int ppbn[3] = {160, 128, 256};
  static const int ppbm[2] = {256, 192};
  for (int bi = 0; bi < 2; ++bi)
    for (int ci = 0; ci < 3; ++ci) {
      const int bm = ppbm[bi], bn = ppbn[ci];
      if (!family_admits(V_PP, p, {bm, bn, 1}) || p.M <= 256) continue;
      for (int sk = 1; sk <= 32; sk *= 2) {        // (round 4: up to 32 -- at the 16 x 16 level a 256-row tile halves the weight re-reads per CU, and only a deep split fills the chip with it)
        if (sk > 1 && !can_split(sk, V_PP)) break;
        long long blocks = tiles(bm, bn) * sk;
        if (blocks < 128) continue;
        if (sk > 1 && blocks > 1024) break;
        add({bm, bn, sk}, V_PP, 2);
      }
    }
  // its patch form: 192 x {160, 128} tiles, one launch
  for (int ci = 0; ci < 2; ++ci)
    if (family_admits(V_PP3, p, {192, ppbn[ci], 1}) && (long long)(p.M / 192) * ((p.N + ppbn[ci] - 1) / ppbn[ci]) >= 128) add({192, ppbn[ci], 1}, V_PP3, 2);
  // the persistent short-K kernel: a candidate once its 128 x 128 tiles occupy a good part of the CUs (with fewer tiles than
  // blocks it is simply a 4-wave kernel with a register epilogue: 8192 x 320 x 320 8.2 vs 9.0 us, 2048 x 1920 x 640 12.0 vs 13.6)
  if (family_admits(V_C4, p, {128, 128, 1}) && tiles(128, 128) >= 96) add({128, 128, 1}, V_C4, 2);
  // the activation-resident short-K kernel (K = 256 / 320): the tile order is its own (n fastest inside a block's run)
  if (family_admits(V_AR, p, {128, 128, 1}) && tiles(128, 128) >= 96) add({128, 128, 1}, V_AR, 1);
  // the 256-row persistent short-K kernel: one 8-wave block per CU walks 256 x 128 tiles.  MEASURED SLOWER than k_gemm_c4 on every shape it was
  // built for (profiles/r05_c8_bench.txt: 5-20 %: eight waves in lockstep idle the matrix pipe during every epilogue, where k_gemm_c4's two independent blocks
  // overlap one's epilogue with the other's K loop), so the tuner tries it only when asked (TF_TUNE_C8=1); table rows and tf_gemm_debug(16384) still select it
  static const bool tune_c8 = getenv("TF_TUNE_C8") != nullptr;
  if (tune_c8 && family_admits(V_C8, p, {256, 128, 1}) && tiles(256, 128) >= 192) add({256, 128, 1}, V_C8, 2);
  return out;
}

static int autotune(const GemmP& p, void* workspace, size_t workspace_bytes, hipStream_t st, TunedCfg* out) {
  TunedCfg bc = p.mx ? mx_default(p) : p.gi_part ? gi_default(p) : TunedCfg{choose_tiles(p.M, p.N, p.K, p.act, true), V_RING, 0};   // stands when nothing beats it
  float best = 1e30f;
  for (const Candidate& k : tune_candidates(p, workspace, workspace_bytes)) {
    GemmP q = p;
    if (k.drop_gn_stats) q.gn_part = nullptr;
    float ms = 0.f;
    int rc = time_config(q, k.c, k.variant, k.order, workspace, st, &ms);
    if (rc) return rc;
    if (ms < best) { best = ms; bc = {k.c, k.variant, k.order}; }
  }
  *out = bc;
  return TF_OK;
}
