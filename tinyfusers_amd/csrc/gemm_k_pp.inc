// Launcher of one k_igemm_pp instance, included by gemm_k_pp16.hip (fp16) and gemm_k_pp8.hip (e4m3).
#include "gemm_pp.h"

template <int BN, int NP, bool FASTA, bool F8 = false, bool H2 = false, int BM = 256, bool LNF = false>
static int launch_pp2(const GemmP& p, hipStream_t st) {
  constexpr int smem = PpLds<BM, BN, F8, H2>::total;        // the layout the kernel reads (gemm_pingpong.h)
  static_assert(smem <= 163840, "LDS budget");
#ifdef TF_ABLATION
  if constexpr (!F8 && FASTA && BM == 256 && !LNF) {       // ablation build (tools/pp_dbg.py): the lean-addressing fp16 instances only
    if (p.dbg) {
      static bool attr_dbg = false;
      if (!attr_dbg) {
        TF_HIP(hipFuncSetAttribute((const void*)k_igemm_pp<BN, NP, FASTA, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
        attr_dbg = true;
      }
      hipLaunchKernelGGL((k_igemm_pp<BN, NP, FASTA, true>), dim3(p.ntm * p.ntn * p.splitk), dim3(512), smem, st, p);
      TF_LAUNCH_CHECK();
      return TF_OK;
    }
  }
#endif
  static bool attr_set = false;
  if (!attr_set) {
    TF_HIP(hipFuncSetAttribute((const void*)k_igemm_pp<BN, NP, FASTA, false, F8, H2, BM, LNF, kBF>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840));
    attr_set = true;
  }
  hipLaunchKernelGGL((k_igemm_pp<BN, NP, FASTA, false, F8, H2, BM, LNF, kBF>), dim3(p.ntm * p.ntn * p.splitk), dim3(512), smem, st, p);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
