// The GEMM kernel families as the dispatcher sees them: their names, which launches each can take, and one fully specified launch.
// Host side only (included by gemm.hip): the kernels and their launchers are gemm_common.h's and the gemm_k_*.hip translation units'.
#pragma once
#include "gemm_reduce.h"

// The values are the `variant` column of the tuning table (gemm_tune_gfx950.txt), of tf_prof_dump's CSV and of tf_gemm_tune_query / _entry: frozen.
enum Variant {
  V_NONE = -1,
  V_RING = 0,    // k_igemm, deep ring (k_igemm8 for fixed-scale e4m3 operands)
  V_WIDE = 1,    // k_igemm, two blocks per CU
  V_PATCH = 2,   // k_igemm_patch; a launch it cannot take runs the deep ring
  V_ALL8 = 3,    // k_igemm, deep ring, the consumer waves issue part of the weight pieces; the deep ring itself for channel counts off the 64 grid
  V_PP = 4,      // k_igemm_pp, the ping-pong kernel
  V_C4 = 5,      // k_gemm_c4, the persistent short-K kernel
  V_PP3 = 6,     // k_igemm_pp3, the patch form of the ping-pong kernel
  V_C8 = 7,      // k_gemm_c8, the 256-row persistent short-K kernel
  V_AR = 8,      // k_gemm_ar, the activation-resident short-K kernel
  V_COUNT
};
struct TileCfg { int bm, bn, splitk; };

static int g_part16 = 1;                                  // split-K partial slabs in fp16 (tf_gemm_splitk_partials: 16 / 32)
static int g_slab_gm = 1;                                 // group-major split-K slabs where the fused reduce finishes the launch (tf_gemm_splitk_slab_layout: 0 / 1)
static int g_pp_np = 0;                                    // test / tuning hook: 0 = default phases per K tile, 2 = one phase per k-step where the tile has both forms

// GroupNorm statistics from the producing conv: limits shared by the host entry, the tuner and the launches
#define TF_GN_MAX_CHUNKS 192    // (192: a 128-wide tile on 96 x 96 outputs emits 2 pieces x 96 half-tile chunks per image: the block-scaled patch kernel at config 5's first level)
static int gn_reduce_chunks(int HoWo) { int R = (HoWo + TF_GN_MAX_CHUNKS - 1) / TF_GN_MAX_CHUNKS; while (HoWo % R) ++R; return HoWo / R; }
static int gn_pieces(const GemmP& p, int bn) { return bn % p.gn_cpg == 0 ? 1 : 2; }   // chunks per m-tile (igemm_gn_stats)
static int gn_chunks_for(const GemmP& p, TileCfg c, int splitk) {
  return splitk > 1 ? gn_reduce_chunks(p.HoWo) : gn_pieces(p, c.bn) * (p.HoWo / c.bm);
}
static bool gn_tile_ok(const GemmP& p, int bm, int bn) { return p.HoWo % bm == 0 && gn_pieces(p, bn) * (p.HoWo / bm) <= TF_GN_MAX_CHUNKS; }

// ---- what each kernel needs of a launch ----------------------------------------------------------------------------------------------
// k_igemm_patch: eligibility + geometry for a (bm, bn) tile.  3x3 / stride 1 / pad 1, no up-sampling, every channel count a
// multiple of 64, W a power of two that divides bm, m-tiles inside one image, and an LDS budget that leaves >= 3 ring slots.
static bool patch_setup(GemmP& p, int bm, int bn) {
  if (p.act || p.ln_colsum || p.S != 3 || p.Kc != 9 * p.C || p.stride != 1 || p.pad != 1 || p.ups) return false;
  if ((p.C1 % 64) || (p.C2 % 64) || (p.C3 % 64) || (p.C4 % 64) || p.H != p.Ho || p.W != p.Wo) return false;
  if (!((bm == 64 || bm == 128) && (bn == 128 || bn == 160))) return false;
  if ((p.W & (p.W - 1)) || p.W < 8 || p.W > bm || p.HoWo % bm) return false;
  int l2 = 0;
  while ((1 << l2) < p.W) ++l2;
  const int ppix = (bm / p.W + 2) * (p.W + 2), ppc = (ppix + 7) / 8;
  if ((ppc + 3) / 4 > TF_PATCH_PPW) return false;
  const int stage = bn * 128 + ((p.C3 + p.C4) ? bm * 128 : 0);
  int ns = (163840 - 2 * ppc * 1024 - gi_table_bytes(p)) / stage;
  if (ns > 5) ns = 5;                                    // patch pieces ride from tap 4 on: needs ns - 1 <= 4 (k_igemm_patch TAP0)
  if (ns < 3) return false;
  p.pt_ppc = ppc; p.pt_ppix = ppix; p.pt_stage = stage; p.pt_ns = ns; p.pt_log2w = l2;
  p.gi_off = 2 * ppc * 1024 + ns * stage;
  return true;
}
// ... asked as a question: would k_igemm_patch take this tile of the launch?
static bool patch_admits(const GemmP& p, int bm, int bn) { GemmP probe = p; return patch_setup(probe, bm, bn); }
// k_igemm_pp: 256 x BN tiles, every channel count on the 64 grid, no LayerNorm fold, no input GroupNorm, fp16 only
static bool pp_ok(const GemmP& p, int bn, int bm = 256) {
  if (bn != 128 && bn != 160 && bn != 256) return false;
  if (bm != 256 && !(bm == 192 && bn != 256)) return false;
  if ((p.bf16 && p.fp8) || p.gi_part || gemm_generic(p)) return false;
  if (p.ln_colsum && (p.fp8 || p.S != 1 || p.stride != 1 || p.ups)) return false;   // the LayerNorm fold: linears, fp16
  if (p.fp8) {
    // the e4m3 form: block-scaled activations only, the lean addressing only (stride 1, no up-sampling), a whole K tile's fragments in
    // registers (three-slot ring: no 256-wide tile), and room for the scale table behind the ring (not 256 x 160 with half-tile slabs)
    if (!p.mx || bn == 256 || !pp_fast(p) || p.C3 || p.C4) return false;
    const bool h2 = (p.C1 % 128) || (p.C2 % 128);
    if (bm == 256 && bn == 160 && h2) return false;
    if (p.out8 && !(p.act == 1 && bn == 128)) return false;   // a block-scaled output: the GEGLU epilogue of the 128-wide tile
  }
  if (p.bias_nc && p.HoWo < bm) return false;            // the epilogue's time-embedding table holds two images per tile
  return p.act != 1 || bn % 64 == 0;                     // GEGLU pairs 16-row value | gate blocks inside a wave tile
}
// k_igemm_pp3: the PATCH form of the ping-pong kernel -- 3x3 / stride 1 / pad 1 convolutions of fp16 operands, every channel count on
// the 64 grid, a 192-row tile that is a whole number of image rows inside one image (W | 192, 192 | H W: the 96 / 48 / 24-pixel levels of
// BASELINE config 5, the OUTPUT row length a template parameter; nearest-2x up-sampling folds into the patch gather), no split-K; fp16, or block-scaled
// e4m3 on the 128-channel grid; two patch buffers + three weight slots in LDS.  (A question only: the kernel takes its geometry from GemmP as it is.)
static int pp3_bn(const GemmP& p) { return (p.Wo == 96 && !p.fp8) ? 160 : 128; }                        // the instantiated (output row length, tile width) pairs
static bool pp3_setup(const GemmP& p, int bm, int bn) {
  if (bm != 192 || bn != pp3_bn(p)) return false;
  if ((p.bf16 && p.fp8) || p.gi_part || p.ln_colsum || p.act || p.out8 || p.out32 || gemm_generic(p)) return false;
  // e4m3: block-scaled, 128-channel slabs; a channel count on the 64 grid (one source tensor, its last slab half full) has instances for 96 / 48-pixel rows
  if (p.fp8 && (!p.mx || ((p.C1 % 128) && (p.C2 || p.Wo == 24)) || (p.C2 % 128))) return false;
  if (p.S != 3 || p.Kc != 9 * p.C || p.K != p.Kc + p.C3 + p.C4 || p.stride != 1 || p.pad != 1) return false;
  if ((p.C3 || p.C4) && (p.fp8 || p.ups || (p.C3 % 64) || (p.C4 % 64))) return false;               // the folded 1x1 skip projection: fp16, its sources at output resolution
  if ((p.C1 % 64) || (p.C2 % 64) || (p.H << p.ups) != p.Ho || (p.W << p.ups) != p.Wo) return false;   // (nearest-2x up-sampling folds into the patch gather)
  if ((p.Wo != 96 && p.Wo != 48 && p.Wo != 24) || (p.HoWo % 192) || (p.M % p.HoWo)) return false;   // the instantiated row lengths; a tile = whole rows of one image
  return true;
}
// k_gemm_c4: the persistent short-K kernel -- linears / 1x1 stride-1 convolutions of fp16 operands whose channel counts sit on
// the 64 grid, one launch (no split-K), no statistics, no time-embedding bias; bias, residual, GEGLU and the LayerNorm fold ride along
static bool c4_ok(const GemmP& p) {
  if (p.fp8 || p.gi_part || p.gn_part || p.bias_nc || p.out32 || p.out8 || p.on_z) return false;
  if (p.S != 1 || p.stride != 1 || p.pad != 0 || p.ups || p.C3 || p.C4 || p.K != p.Kc) return false;
  if ((p.C1 % 64) || (p.C2 % 64) || (p.N % 8) || p.M < 1) return false;
  return p.act == 0 || (p.act == 1 && p.N % 64 == 0);
}
// k_gemm_ar: the activation-resident short-K kernel -- k_gemm_c4's launches whose K is 4 or 5 whole K tiles (256 / 320: the 128-row panel stays in LDS), no residual
static bool ar_ok(const GemmP& p) { return c4_ok(p) && (p.K == 256 || p.K == 320) && !p.residual; }   // (its loader waves store the outputs: a residual would be a second load stream in their instruction budget -- those launches stay on k_gemm_c4)

// GroupNorm of the input inside the launch (gi): which (tile, variant) can carry it.  3x3 / stride 1 / pad 1: the PATCH kernel only
// (a piece is normalised once for its nine taps); 1x1: the tap-by-tap kernel (k = channel), any ring variant; every channel count on
// the 64 grid, m-tiles inside one image (one statistics table per block), and room in LDS for the table.
static bool gi_tile_ok(const GemmP& p, int bm, int bn, int variant) {
  if (!p.gi_part) return true;
  if (gemm_generic(p) || p.act || p.ln_colsum || p.HoWo % bm) return false;
  if (p.S == 3) return variant == V_PATCH && patch_admits(p, bm, bn);
  if (p.S != 1 || p.Kc != p.C || p.stride != 1 || p.pad != 0 || p.ups) return false;
  if (variant == V_PATCH || (bm == 128 && bn == 160)) return false;
  return ((igemm_lds_bytes(bm, bn, variant == V_WIDE) + 15) & ~15) + gi_table_bytes(p) <= 163840;
}
static bool gi_any_ok(const GemmP& p) {
  static const int cand[][2] = {{128, 160}, {64, 160}, {128, 128}, {64, 128}, {128, 64}, {64, 64}};
  for (int ci = 0; ci < 6; ++ci)
    for (int v = V_RING; v <= V_ALL8; ++v)
      if (gi_tile_ok(p, cand[ci][0], cand[ci][1], v)) return true;
  return false;
}

// ---- the families: everything the dispatcher knows about one, once ------------------------------------------------------------------------
#define TF_BF(p, fn, ...) ((p).bf16 ? fn##_bf16(__VA_ARGS__) : fn(__VA_ARGS__))      /* the bfloat16 twin of a launcher */
// the k_igemm forms share one admission rule and one launcher table; fixed-scale e4m3 operands have k_igemm8, a deep ring, whichever form was asked for
static bool ring_admits(const GemmP& p, int bm, int bn, int, int variant) { return !(p.bf16 && p.fp8) && !p.mx && gi_tile_ok(p, bm, bn, variant); }
static int ring_launch(GemmP& p, hipStream_t st, int bm, int bn, int variant) {
  const bool wide = variant == V_WIDE, all8 = variant == V_ALL8;
  if (p.fp8) return tfk_launch_igemm8(p, st, bm, bn);
  if (bm == 256 && bn == 128) return TF_BF(p, tfk_launch_igemm_256x128, p, st);
  if (bn == 160) return TF_BF(p, tfk_launch_igemm_160, p, st, bm, wide, all8);
  if (bn == 128) return TF_BF(p, tfk_launch_igemm_128, p, st, bm, wide, all8);
  if (bn == 64) return TF_BF(p, tfk_launch_igemm_64, p, st, bm, wide, all8);
  tf_set_error("run_gemm: no kernel for tile %dx%d", bm, bn);
  return TF_E_UNSUPPORTED;
}
struct Family {
  const char* name;                                       // for error texts
  bool pingpong;                                          // K tiles of 128 e4m3 elements (64 fp16 ones: 128 BYTES of a row, like every other family); the statistics epilogue works in half-tile sub-blocks
  bool (*admits)(const GemmP& p, int bm, int bn, int sk, int variant);   // may the family run tile bm x bn of p with an (effective) split sk?  A question: p is not changed
  int (*launch)(GemmP& p, hipStream_t st, int bm, int bn, int variant);  // an admitted launch (fills the geometry the kernel wants into p)
  // what the resolver (gemm.hip: settle_variant) does with the family:
  TileCfg (*own_tile)(const GemmP& p);                    // the one tile the kernel has for p; nullptr: the tiles admits() accepts
  bool forced_tile_first;                                 // tf_gemm_force_config's tile, where it differs from own_tile, counts as "cannot take it" (else own_tile replaces it)
  int fallback;                                           // the family a table row it cannot take runs on instead; V_NONE: launch_one reports the failure
  int retile_rows;                                        // ... with the cost model's tile again when the row's tile has at least this many rows (0: always; -1: the tile stays)
};
static const Family kFamily[V_COUNT] = {
  /* V_RING  */ {"deep ring", false, ring_admits, ring_launch, nullptr, false, V_NONE, -1},
  /* V_WIDE  */ {"wide ring", false, ring_admits, ring_launch, nullptr, false, V_NONE, -1},
  /* V_PATCH */ {"patch", false, ring_admits,           // (admitted like the deep ring, which runs what patch_setup refuses)
                 [](GemmP& p, hipStream_t st, int bm, int bn, int) {
                   return !p.fp8 && patch_setup(p, bm, bn) ? TF_BF(p, tfk_launch_patch, p, st, bm, bn) : ring_launch(p, st, bm, bn, V_RING);
                 },
                 nullptr, false, V_NONE, -1},
  /* V_ALL8  */ {"all8 ring", false, ring_admits, ring_launch, nullptr, false, V_NONE, -1},
  /* V_PP    */ {"ping-pong", true,
                 [](const GemmP& p, int bm, int bn, int, int) { return pp_ok(p, bn, bm); },
                 [](GemmP& p, hipStream_t st, int bm, int bn, int) {
                   return p.fp8 ? tfk_launch_pp8(p, st, bm, bn) : TF_BF(p, tfk_launch_pp16, p, st, bm, bn, g_pp_np);
                 },
                 nullptr, false, V_RING, 192},
  /* V_C4    */ {"persistent short-K", false,
                 [](const GemmP& p, int bm, int bn, int sk, int) { return bm == 128 && bn == 128 && sk == 1 && c4_ok(p); },
                 [](GemmP& p, hipStream_t st, int, int, int) { return TF_BF(p, tfk_launch_c4, p, st); },
                 [](const GemmP&) { return TileCfg{128, 128, 1}; }, true, V_RING, -1},
  /* V_PP3   */ {"ping-pong patch", true,
                 [](const GemmP& p, int bm, int bn, int sk, int) { return sk == 1 && pp3_setup(p, bm, bn); },
                 [](GemmP& p, hipStream_t st, int, int bn, int) { return TF_BF(p, tfk_launch_pp3, p, st, bn); },
                 [](const GemmP& p) { return TileCfg{192, pp3_bn(p), 1}; }, false, V_RING, 192},
  /* V_C8    */ {"256-row persistent short-K", false,
                 [](const GemmP& p, int bm, int bn, int sk, int) { return bm == 256 && bn == 128 && sk == 1 && c4_ok(p); },
                 [](GemmP& p, hipStream_t st, int, int, int) { return TF_BF(p, tfk_launch_c8, p, st); },
                 [](const GemmP&) { return TileCfg{256, 128, 1}; }, true, V_RING, 0},
  /* V_AR    */ {"activation-resident short-K", false,
                 [](const GemmP& p, int bm, int bn, int sk, int) { return bm == 128 && bn == 128 && sk == 1 && ar_ok(p); },
                 [](GemmP& p, hipStream_t st, int, int, int) { return TF_BF(p, tfk_launch_ar, p, st); },
                 [](const GemmP&) { return TileCfg{128, 128, 1}; }, true, V_C4, -1},   // (a table row of another K: the persistent kernel it grew out of)
};
static bool family_admits(int variant, const GemmP& p, TileCfg c) { return kFamily[variant].admits(p, c.bm, c.bn, c.splitk, variant); }

// K tiles of a launch: 64 elements, except the e4m3 ping-pong kernel's 128 (128 BYTES of a row either way).  Everything that reasons about
// split-K -- the effective split count, whether a reduce launch follows, the tuner's "at least 4 K tiles per split" -- goes through this
static int ktiles_for(const GemmP& p, int variant) { return (kFamily[variant].pingpong && p.fp8) ? (p.K + 127) / 128 : (p.K + 63) / 64; }
// rows of a tile as the GroupNorm-statistics code sees them: the ping-pong kernel's epilogue works in 128-row sub-blocks
static int stats_bm(int bm, int variant) { return kFamily[variant].pingpong ? bm / 2 : bm; }
// the split count a launch really runs with (launch_one rounds the requested one to whole K tiles)
static int eff_splitk(const GemmP& p, int variant, int splitk) {
  const int kt = ktiles_for(p, variant), kps = (kt + splitk - 1) / splitk;
  return (kt + kps - 1) / kps;
}

static hipEvent_t g_prof_end = nullptr;   // profiling pass only (gemm_prof.h): recorded right behind the GEMM kernel, in front of its split-K reduce
// one fully specified launch (tile, split-K, family) of the kernel family (+ the split-K reduce)
static int launch_one(GemmP p, TileCfg c, int variant, int order, void* workspace, hipStream_t st) {
  const Family& f = kFamily[variant];
  p.order = order;
  p.ktiles = ktiles_for(p, variant);
  p.ktiles_per_split = (p.ktiles + c.splitk - 1) / c.splitk;
  p.splitk = (p.ktiles + p.ktiles_per_split - 1) / p.ktiles_per_split;
  p.partial = (float*)workspace;
  p.part16 = (g_part16 && !p.bf16 && p.splitk > 1 && (p.N & 7) == 0) ? 1 : 0;     // 16-byte rows segments of halves; other widths -- and the bfloat16 launches, whose partials may leave fp16's range -- keep fp32 slabs
  // group-major slabs (GemmP::slab_gm): where k_splitk_reduce_gn_apply finishes the launch, a quad never straddles a group, and the family's epilogue
  // writes the layout -- k_igemm in its ring forms and k_igemm_patch (fp16 / bfloat16 operands).  Every other family and reducer: row-major
  const bool gm_family = (variant == V_RING || variant == V_WIDE || variant == V_PATCH || variant == V_ALL8) && !p.fp8;
  p.slab_gm = (g_slab_gm && p.splitk > 1 && gm_family && p.on_z && p.gn_part && (p.gn_cpg & 3) == 0 && (long long)p.M * p.N < (1LL << 31) &&
               tfk_splitk_reduce_applies_gn(p.HoWo, p.N, p.gn_G)) ? 1 : 0;      // (M N < 2^31: the epilogue forms the offset inside a slab in 32 bits)
  if (p.slab_gm) fast_div_magic((unsigned)p.gn_cpg, &p.dv_cpg_mul, &p.dv_cpg_shr);
  p.ntm = (p.M + c.bm - 1) / c.bm;
  p.ntn = (p.N + c.bn - 1) / c.bn;
  float* gn_part = p.gn_part;
  if (gn_part) {
    // chunk geometry of the statistics partials: in-kernel (2 pieces per m-tile) or in the split-K reduce (row stripes)
    if (p.splitk > 1) { p.gn_chunks = gn_reduce_chunks(p.HoWo); p.gn_part = nullptr; }
    else p.gn_chunks = gn_pieces(p, c.bn) * (p.HoWo / stats_bm(c.bm, variant));
  }
  if (!f.admits(p, c.bm, c.bn, p.splitk, variant)) {
    tf_set_error("run_gemm: the %s kernel cannot run this launch (tile %dx%d, split %d; M=%d N=%d K=%d, e4m3 %d block-scaled %d bfloat16 %d, input GroupNorm %d)",
                 f.name, c.bm, c.bn, p.splitk, p.M, p.N, p.K, p.fp8, p.mx, p.bf16, p.gi_part ? 1 : 0);
    return TF_E_UNSUPPORTED;
  }
  int rc = f.launch(p, st, c.bm, c.bn, variant);
  if (rc) return rc;
  if (g_prof_end) { TF_HIP(hipEventRecord(g_prof_end, st)); g_prof_end = nullptr; }   // the bracket holds k_igemm* alone (what rocprofv3 lists under that name)
  p.gn_part = gn_part;
  return tfk_launch_splitk_reduce(p, st);
}
