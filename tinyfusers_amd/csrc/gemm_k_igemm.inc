// Launchers of k_igemm instances, included by gemm_k_igemm_{160,128,64}.hip (one translation unit per tile width).
#include "gemm_igemm.h"

template <int BM, int BN, bool GENERIC, bool WIDE, bool ALL8 = false>
static int launch_cfg3(const GemmP& p, hipStream_t st) {
  constexpr int TM = BM / 2, TN = BN / 2;
  constexpr int ring = (WIDE ? 2 : ring_slots(BM, BN)) * (BM + BN) * 128;
  constexpr int scratch = 4 * TM * (TN + 4) * 4;         // epilogue transpose scratch overlays the ring
  constexpr int tail = BM * 8 + 4 * BN * 8;              // LayerNorm (mean, rstd) table + GroupNorm column-sum table behind the scratch
  constexpr int smem = ring > scratch + tail ? ring : scratch + tail;
  static bool attr_set = false;
  if (!attr_set) {
    TF_HIP(hipFuncSetAttribute((const void*)k_igemm<BM, BN, GENERIC, WIDE, ALL8, false, kBF>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    attr_set = true;
  }
  if (p.gi_part) {                                       // the (mean, rstd) + (a, b) table of the input's GroupNorm sits behind everything else
    GemmP q = p;
    q.gi_off = (smem + 15) & ~15;
    const int total = q.gi_off + gi_table_bytes(p);
    if constexpr (GENERIC || (BM == 128 && BN == 160) || BM == 256) {
      tf_set_error("k_igemm<%d,%d>: this instance cannot carry the input GroupNorm", BM, BN); return TF_E_UNSUPPORTED;
    } else {
      if (total > 163840) { tf_set_error("k_igemm<%d,%d>: no room for the GroupNorm table (%d B)", BM, BN, total); return TF_E_UNSUPPORTED; }
      static bool attr_gi = false;
      if (!attr_gi) {
        TF_HIP(hipFuncSetAttribute((const void*)k_igemm<BM, BN, GENERIC, WIDE, ALL8, true, kBF>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
        attr_gi = true;
      }
      hipLaunchKernelGGL((k_igemm<BM, BN, GENERIC, WIDE, ALL8, true, kBF>), dim3(p.ntm * p.ntn * p.splitk), dim3(512), total, st, q);
      TF_LAUNCH_CHECK();
      return TF_OK;
    }
  }
  hipLaunchKernelGGL((k_igemm<BM, BN, GENERIC, WIDE, ALL8, false, kBF>), dim3(p.ntm * p.ntn * p.splitk), dim3(512), TF_IGEMM_STAMP == 2 ? 163840 : smem, st, p);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
template <int BM, int BN, bool WIDE_OK>
static int launch_cfg(const GemmP& p, hipStream_t st, bool wide, bool all8 = false) {
  static_assert(WIDE_OK == igemm_wide_ok(BM, BN), "the instantiated wide forms and igemm_wide_ok disagree");
  bool generic = gemm_generic(p);
  const int form = igemm_ring_form(BM, BN, wide, all8, generic);     // (gemm_common.h: the rule tf_gemm_ring_form answers with)
  if (form == 3) return launch_cfg3<BM, BN, false, false, true>(p, st);
  if (WIDE_OK && form == 1) return generic ? launch_cfg3<BM, BN, true, WIDE_OK>(p, st) : launch_cfg3<BM, BN, false, WIDE_OK>(p, st);
  return generic ? launch_cfg3<BM, BN, true, false>(p, st) : launch_cfg3<BM, BN, false, false>(p, st);
}
