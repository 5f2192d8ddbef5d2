// Scaled-dot-product attention, the plain launch: tf_sdpa_f16 / tf_sdpa_16, the rule that picks a kernel family for a shape (tf_sdpa_instance,
// tf_sdpa_split_ks, tf_sdpa_force_split) and the TF_SDPA_* environment toggles.  The kernels: k_sdpa_dma (sdpa_dma.h), k_sdpa (sdpa_generic.h) and,
// in a unit of their own, the key-slice forms (sdpa_split.hip).  sdpa_bf16.hip compiles this file once more for bfloat16 (TF_TU_BF, common.h).
#include "sdpa_dma.h"
#include "sdpa_generic.h"

static bool g_sdpa_generic = getenv("TF_SDPA_GENERIC") != nullptr;
#ifdef TF_ABLATION
static int g_sdpa_dbg = getenv("TF_SDPA_DBG") ? atoi(getenv("TF_SDPA_DBG")) : 0;   // ablation of k_sdpa_dma<40, 2> (see SdpaP::dbg)
#else
static const int g_sdpa_dbg = 0;   // the shipped library ignores TF_SDPA_DBG: it holds no kernel that returns wrong results
#endif
static int g_sdpa_nw = getenv("TF_SDPA_NW") ? atoi(getenv("TF_SDPA_NW")) : 0;      // A/B: 4 / 8 waves per block where both exist (0 = per-shape choice)
static int g_sdpa_qt = getenv("TF_SDPA_QT") ? atoi(getenv("TF_SDPA_QT")) : 0;   // debugging: force the register-staged kernel
static int g_sdpa_ks = getenv("TF_SDPA_KS") ? atoi(getenv("TF_SDPA_KS")) : 0;   // A/B: key slices inside the block: 0 = per-shape choice, 1 = never, 2 = wherever a split form exists
extern int g_sdpa_force_ks;                                                      // tf_sdpa_force_split (tests): the same three values, in front of TF_SDPA_KS

// Which split form (SDPA_SPLIT_*, 0 = none) a launch takes: from the shape alone, so eager and captured launches of a shape run the same kernel.
// A form exists for the two SD head sizes whose rings fit twice (d = 40, 80; d = 160: 2 x 2 x 43 KiB does not), never under the causal mask (the
// slices' tile ranges would depend on the query block).  Chosen when the unsplit grid leaves a SIMD short of four waves AND the split form adds
// waves to it (d = 40: the eight-wave instance at one block per CU; d = 80: the 16-query instance at one block per CU) AND every slice gets two
// tiles.  ks = 2 (forced) asks only whether a form exists: other head sizes and causal launches stay unsplit.  The per-shape choice also steps aside
// when TF_SDPA_NW / TF_SDPA_QT / TF_SDPA_DBG name an unsplit instance.
static int sdpa_split_form(int B, int NH, int Tq, int Tk, int HS, int causal, bool small) {
  const int ks = g_sdpa_force_ks ? g_sdpa_force_ks : g_sdpa_ks;
  if (ks == 1 || causal || !small || g_sdpa_generic || (HS != 40 && HS != 80)) return 0;
  const int form = HS == 40 ? SDPA_SPLIT_40_W16 : SDPA_SPLIT_80_Q16;
  if (ks >= 2) return form;
  if (g_sdpa_nw || g_sdpa_qt || g_sdpa_dbg) return 0;
  const int ntiles = (Tk + 63) / 64;
  if (ntiles < 4) return 0;                                                      // two slices of at least two tiles
  const long long blocks8 = (long long)((Tq + 255) / 256) * NH * B, blocks1 = (long long)((Tq + 63) / 64) * NH * B;
  // d = 40: the unsplit launch is <40, 2, 8> (blocks8 >= 256); up to 256 blocks it puts 8 waves on a CU, two per SIMD, and 16-wave blocks make that four
  if (HS == 40) return blocks8 >= 256 && blocks8 * 8 < 4 * 1024 ? form : 0;
  // d = 80: the unsplit launch is <80, 1> (fewer than 256 blocks of 128 queries) at one block per CU (84 KiB of ring): one wave per SIMD, split two
  const long long blocks2 = (long long)((Tq + 127) / 128) * NH * B;
  return blocks2 < 256 && blocks1 <= 256 ? form : 0;
}
// the rule once the split forms are left out, which the dual and the perturbed launch (sdpa_dual.hip, sdpa_pag.hip: no split forms) ask for on its own
static int sdpa_instance_unsplit(int B, int NH, int Tq, int HS) {
  if (g_sdpa_generic || (HS != 40 && HS != 64 && HS != 80 && HS != 128 && HS != 160)) return TF_SDPA_INST_GENERIC;
  // 16 queries per wave (QT = 1) doubles the waves in flight; g_sdpa_qt: 0 = per-shape choice, 1 / 2 forced (TF_SDPA_QT)
  // (measured: 32x32 d80 22.5 -> 19.7 us, 16x16 d160 13.4 -> 10.6 us with 16-query waves; 64x64 d40 93.8 -> 118.7 us: only when
  // the 32-query grid would leave CUs without a block)
  const long long blocks2 = (long long)((Tq + 127) / 128) * NH * B;
  const bool narrow = g_sdpa_qt ? g_sdpa_qt == 1 : blocks2 < 256;
  if (narrow) return TF_SDPA_INST_DMA16;
  // eight waves per block (256 queries per K/V tile fetch) once that still gives every CU a block (measured: 64 x 64 d40, B 2: 86.9 -> 81.0 us
  // with ONE eight-wave block per CU; 96 x 96, B 8: 1214 -> 1103 us)
  const long long blocks8 = (long long)((Tq + 255) / 256) * NH * B;
  const bool wide8 = g_sdpa_nw ? g_sdpa_nw == 8 : blocks8 >= 256;
  return wide8 && (HS == 40 || HS == 80) ? TF_SDPA_INST_DMA32_W8 : TF_SDPA_INST_DMA32;
}
// Which kernel family a launch runs (TF_SDPA_INST_* of include/tinyfusers_hip.h), from the shape and the K / V token strides alone; 0 = no kernel
// can run it.  THE rule: sdpa_run branches on this value and tf_sdpa_instance returns it.  *form: the SDPA_SPLIT_* of a split launch.
enum { SDPA_INST_NONE = 0 };     // (not one of tfSdpaInstance's values)
static int sdpa_instance(int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int causal, int* form) {
  const bool small = sdpa_addressable(Tk, HS, k_st, v_st);
  *form = 0;
  if (!small) return SDPA_INST_NONE;
  if ((*form = sdpa_split_form(B, NH, Tq, Tk, HS, causal, small))) return TF_SDPA_INST_SPLIT;
  return sdpa_instance_unsplit(B, NH, Tq, HS);
}
// the query behind tf_sdpa_instance, in this unit's element type (each unit asks its own copy of the rule: the one its launcher branches on)
int tfk_sdpa_instance_bf16(int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int causal);
int TFK(tfk_sdpa_instance)(int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int causal) {
  int form;
  return sdpa_instance(B, NH, Tq, Tk, HS, k_st, v_st, causal, &form);
}

// The launch, with this unit's kernels (kBF): tf_sdpa_f16 here, tfk_sdpa_bf16 in sdpa_bf16.hip.  Both report as tf_sdpa_f16.
static int sdpa_run(SdpaP p, tfStream_t s) {
  const char* who = "tf_sdpa_f16";
  TF_REQUIRE(p.o && p.q && p.k && p.v, "%s: null tensor", who);
  if (int rc = sdpa_check_shape(who, nullptr, p.B, p.NH, p.Tq, p.Tk, nullptr, p.HS, 0)) return rc;
  if (int rc = sdpa_check_launch(who, "q/k/v", p)) return rc;
  if (p.B == 0 || p.Tq == 0) return TF_OK;
  p.dbg = g_sdpa_dbg;
  // the instance is decided (and a slice no kernel can address refused) before anything touches the device
  int form;
  const int inst = sdpa_instance(p.B, p.NH, p.Tq, p.Tk, p.HS, p.k_st, p.v_st, p.causal, &form);
  if (inst == SDPA_INST_NONE) return sdpa_refuse(who, p.Tk, p.HS, p.k_st, p.v_st);
  hipStream_t st = tf_hs(s);
  TfProfScope prof_(TF_PROF_FAM_SDPA, 4.0 * p.B * p.NH * (double)p.Tq * p.Tk * p.HS, st);      // (FLOPs = 4 B NH Tq Tk d)
  if (inst == TF_SDPA_INST_SPLIT) return TFK(tfk_sdpa_split)(p, form, st);
  if (inst == TF_SDPA_INST_DMA16) return sdpa_by_head_size<40, 64, 80, 128, 160>(p.HS, [&](auto hs) { return launch_sdpa_dma<hs, 1>(p, st); });
  if (inst == TF_SDPA_INST_DMA32_W8) return sdpa_by_head_size<40, 80>(p.HS, [&](auto hs) { return launch_sdpa_dma<hs, 2, 8>(p, st); });
  if (inst == TF_SDPA_INST_DMA32) return sdpa_by_head_size<40, 64, 80, 128, 160>(p.HS, [&](auto hs) { return launch_sdpa_dma<hs, 2>(p, st); });
  return launch_sdpa<kBF>(p, st);
}

#if TF_TU_BF
int tfk_sdpa_bf16(const SdpaP& p, tfStream_t s) { return sdpa_run(p, s); }
#else
int tfk_sdpa_bf16(const SdpaP& p, tfStream_t s);
int tfk_sdpa_instance_unsplit(int B, int NH, int Tq, int HS) { return sdpa_instance_unsplit(B, NH, Tq, HS); }
int g_sdpa_force_ks = 0;
extern "C" int tf_sdpa_force_split(int ks) {
  TF_REQUIRE(ks >= 0 && ks <= 2, "tf_sdpa_force_split: ks=%d (0 = per-shape choice, 1 = unsplit, 2 = two key slices)", ks);
  g_sdpa_force_ks = ks;
  return TF_OK;
}
extern "C" int tf_sdpa_split_ks(int B, int NH, int Tq, int Tk, int HS, int causal) {
  return sdpa_split_form(B, NH, Tq, Tk, HS, causal, true) ? 2 : 1;
}
extern "C" int tf_sdpa_instance(int dtype, int B, int NH, int Tq, int Tk, int HS, long long k_st, long long v_st, int causal) {
  if (int rc = sdpa_check_shape("tf_sdpa_instance", &dtype, B, NH, Tq, Tk, nullptr, HS, 1)) return rc;
  const long long str[] = {k_st, v_st};
  if (int rc = sdpa_check_strides("tf_sdpa_instance", "k / v", str, 2)) return rc;
  const int inst = dtype == TF_DTYPE_BF16 ? tfk_sdpa_instance_bf16(B, NH, Tq, Tk, HS, k_st, v_st, causal) : tfk_sdpa_instance(B, NH, Tq, Tk, HS, k_st, v_st, causal);
  return inst ? inst : sdpa_refuse("tf_sdpa_instance", Tk, HS, k_st, v_st);
}

extern "C" int tf_sdpa_f16(void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS, long long q_sb, long long q_sh, long long q_st,
                           long long k_sb, long long k_sh, long long k_st, long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh, long long o_st,
                           int causal, tfStream_t s) {
  return sdpa_run(sdpa_params(o, q, k, v, B, NH, Tq, Tk, HS, q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st, causal), s);
}
extern "C" int tf_sdpa_16(int dtype, void* o, const void* q, const void* k, const void* v, int B, int NH, int Tq, int Tk, int HS, long long q_sb, long long q_sh, long long q_st,
                          long long k_sb, long long k_sh, long long k_st, long long v_sb, long long v_sh, long long v_st, long long o_sb, long long o_sh, long long o_st, int causal,
                          tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_sdpa_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  const SdpaP p = sdpa_params(o, q, k, v, B, NH, Tq, Tk, HS, q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st, causal);
  return dtype == TF_DTYPE_BF16 ? tfk_sdpa_bf16(p, s) : sdpa_run(p, s);
}
#endif
