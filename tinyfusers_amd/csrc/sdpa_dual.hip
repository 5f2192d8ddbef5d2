// Decoupled cross-attention in one launch (tf_sdpa_dual_16; the IP-Adapter's image tokens next to the text tokens, attention/attention.py:35-41 with a
// second key / value set): o = softmax(q k^T / sqrt d) v + s softmax(q k2^T / sqrt d) v2, two independent softmaxes, s one fp32 read from the device.
// k_sdpa_dual is k_sdpa_dma's body with TF_SDPA_BODY_DUAL (sdpa_dma_body.inc): the 1 .. 64 image keys are one more tile of the ring, so the text
// tiles take the path they take in k_sdpa_dma, no score and no intermediate o goes to HBM, and there is no second accumulator set and no extra LDS.
// A translation unit of its own: the code objects of sdpa.hip / sdpa_split.hip stay what they were without it.
#include "sdpa_common.h"

struct SdpaDualP {
  SdpaP p;                                 // the text launch, as tf_sdpa_16 would fill it (causal = 0)
  const half_t* k2; const half_t* v2; const float* scale2;
  int Tk2;
  long long k2_sb, k2_sh, k2_st, v2_sb, v2_sh, v2_st;
};

template <int HS, int QT, int NW, bool BF>
__global__ void __launch_bounds__(NW * 64) k_sdpa_dual(const SdpaDualP pd) {
  constexpr int KS = 1, SR = 0, DBG = 0;
  const SdpaP& p = pd.p;
#define TF_SDPA_BODY_DUAL 1
#include "sdpa_dma_body.inc"
#undef TF_SDPA_BODY_DUAL
}

template <int HS, int QT, int NW = 4>
static int launch_sdpa_dual(const SdpaDualP& pd, hipStream_t st) {
  return launch_sdpa_kernel<k_sdpa_dual<HS, QT, NW, kBF>>(pd, pd.p, sdpa_ring_bytes<HS, NW>(), 16 * NW * QT, NW, st);      // k_sdpa_dma<HS, QT, 0, NW>'s ring
}

int tfk_sdpa_dual_bf16(const SdpaDualP& pd, int inst, hipStream_t st);
int TFK(tfk_sdpa_dual)(const SdpaDualP& pd, int inst, hipStream_t st) {
  if (inst == TF_SDPA_INST_DMA16) return sdpa_by_head_size<40, 80, 160>(pd.p.HS, [&](auto hs) { return launch_sdpa_dual<hs, 1>(pd, st); });
  if (inst == TF_SDPA_INST_DMA32_W8 && pd.p.HS != 160) return sdpa_by_head_size<40, 80>(pd.p.HS, [&](auto hs) { return launch_sdpa_dual<hs, 2, 8>(pd, st); });
  return sdpa_by_head_size<40, 80, 160>(pd.p.HS, [&](auto hs) { return launch_sdpa_dual<hs, 2>(pd, st); });
}

#if !TF_TU_BF
// Which family a dual launch runs (sdpa_unsplit_dma_rule), among the head sizes the dual form is built for; either key set must be addressable
static int sdpa_dual_rule(int B, int NH, int Tq, int Tk, int Tk2, int HS, long long k_st, long long v_st, long long k2_st, long long v2_st) {
  return sdpa_unsplit_dma_rule(B, NH, Tq, HS, sdpa_addressable(Tk, HS, k_st, v_st) && sdpa_addressable(Tk2, HS, k2_st, v2_st));
}
static int sdpa_dual_refuse(const char* who, int rule, int Tk, int Tk2, int HS, long long k_st, long long v_st, long long k2_st, long long v2_st) {
  if (rule == 0) return sdpa_addressable(Tk, HS, k_st, v_st) ? sdpa_refuse(who, Tk2, HS, k2_st, v2_st) : sdpa_refuse(who, Tk, HS, k_st, v_st);
  tf_set_error("%s: the dual form exists for the LDS-DMA families only (TF_SDPA_GENERIC is set)", who);
  return TF_E_UNSUPPORTED;
}
// the checks on sizes and strides shared by the launch and the query; 0 or a status with the message set
static int sdpa_dual_args(const char* who, int dtype, int B, int NH, int Tq, int Tk, int Tk2, int HS, long long k_st, long long v_st, long long k2_st, long long v2_st) {
  if (int rc = sdpa_check_shape(who, &dtype, B, NH, Tq, Tk, &Tk2, HS, 0)) return rc;
  const long long str[] = {k_st, v_st, k2_st, v2_st};
  if (int rc = sdpa_check_strides(who, "k / v / k2 / v2", str, 4)) return rc;
  if (Tk2 > 64) {
    tf_set_error("%s: Tk2=%d: the second key set is one tile of at most 64 keys", who, Tk2);
    return TF_E_UNSUPPORTED;
  }
  if (HS != 40 && HS != 80 && HS != 160) {
    tf_set_error("%s: head size %d: the dual form is built for 40, 80 and 160 (the SD UNets' cross-attentions)", who, HS);
    return TF_E_UNSUPPORTED;
  }
  return TF_OK;
}

extern "C" int tf_sdpa_dual_instance(int dtype, int B, int NH, int Tq, int Tk, int Tk2, int HS, long long k_st, long long v_st, long long k2_st, long long v2_st) {
  if (int rc = sdpa_dual_args("tf_sdpa_dual_instance", dtype, B, NH, Tq, Tk, Tk2, HS, k_st, v_st, k2_st, v2_st)) return rc;
  TF_REQUIRE(B >= 1 && Tq >= 1, "tf_sdpa_dual_instance: bad sizes B=%d Tq=%d", B, Tq);
  const int rule = sdpa_dual_rule(B, NH, Tq, Tk, Tk2, HS, k_st, v_st, k2_st, v2_st);
  return rule > 0 ? rule : sdpa_dual_refuse("tf_sdpa_dual_instance", rule, Tk, Tk2, HS, k_st, v_st, k2_st, v2_st);
}

extern "C" int tf_sdpa_dual_16(int dtype, void* o, const void* q, const void* k, const void* v, int Tk, const void* k2, const void* v2, int Tk2, const float* scale2_dev,
                               int B, int NH, int Tq, int HS, long long q_sb, long long q_sh, long long q_st, long long k_sb, long long k_sh, long long k_st,
                               long long v_sb, long long v_sh, long long v_st, long long k2_sb, long long k2_sh, long long k2_st, long long v2_sb, long long v2_sh,
                               long long v2_st, long long o_sb, long long o_sh, long long o_st, tfStream_t s) {
  const char* who = "tf_sdpa_dual_16";
  TF_REQUIRE(o && q && k && v && k2 && v2 && scale2_dev, "%s: null tensor", who);
  if (int rc = sdpa_dual_args(who, dtype, B, NH, Tq, Tk, Tk2, HS, k_st, v_st, k2_st, v2_st)) return rc;
  SdpaDualP pd;
  pd.p = sdpa_params(o, q, k, v, B, NH, Tq, Tk, HS, q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st, 0);
  pd.k2 = (const half_t*)k2; pd.v2 = (const half_t*)v2; pd.scale2 = scale2_dev; pd.Tk2 = Tk2;
  pd.k2_sb = k2_sb; pd.k2_sh = k2_sh; pd.k2_st = k2_st; pd.v2_sb = v2_sb; pd.v2_sh = v2_sh; pd.v2_st = v2_st;
  const long long str2[] = {k2_sb, k2_sh, v2_sb, v2_sh};
  if (int rc = sdpa_check_launch(who, "q / k / v / k2 / v2", pd.p, str2, 4)) return rc;
  if (B == 0 || Tq == 0) return TF_OK;
  // the instance is decided (and a slice no kernel can address refused) before anything touches the device
  const int rule = sdpa_dual_rule(B, NH, Tq, Tk, Tk2, HS, k_st, v_st, k2_st, v2_st);
  if (rule <= 0) return sdpa_dual_refuse(who, rule, Tk, Tk2, HS, k_st, v_st, k2_st, v2_st);
  hipStream_t st = tf_hs(s);
  TfProfScope prof_(TF_PROF_FAM_SDPA, 4.0 * B * NH * (double)Tq * ((double)Tk + Tk2) * HS, st);
  return dtype == TF_DTYPE_BF16 ? tfk_sdpa_dual_bf16(pd, rule, st) : tfk_sdpa_dual(pd, rule, st);
}
#endif
