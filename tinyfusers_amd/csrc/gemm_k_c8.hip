// k_gemm_c8 instances: the 256-row persistent short-K kernel (csrc/gemm.hip is the host side: c8_ok; gemm_c8.h the kernel, gemm_shortk.h what it shares with k_gemm_c4 / k_gemm_ar)
#include "gemm_c8.h"
int TFK(tfk_launch_c8)(const GemmP& p, hipStream_t st) {
  constexpr int smem = 3 * (256 + 128) * 128 + 8 * 64 * 8;   // the three-slot ring (the epilogue's patches live in the slot the next two K tiles do not use) + the LayerNorm row-sum exchange
  static bool attr_set = false;
  if (int e = shortk_set_lds(attr_set, smem, {(const void*)k_gemm_c8<false, kBF>, (const void*)k_gemm_c8<true, kBF>})) return e;
  const int tiles = p.ntm * p.ntn;
  GemmP q = p;
  q.c4_chunk = shortk_chunk(p, tiles, 4);
  const int chunks = (tiles + q.c4_chunk - 1) / q.c4_chunk;
  const int grid = chunks < shortk_num_cus() ? chunks : shortk_num_cus();   // one resident 8-wave block per CU walks the tile list
  if (p.ln_colsum) hipLaunchKernelGGL((k_gemm_c8<true, kBF>), dim3(grid), dim3(512), smem, st, q);
  else hipLaunchKernelGGL((k_gemm_c8<false, kBF>), dim3(grid), dim3(512), smem, st, q);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
