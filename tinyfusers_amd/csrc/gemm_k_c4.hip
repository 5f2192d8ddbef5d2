// k_gemm_c4 instances: the persistent short-K kernel (csrc/gemm.hip is the host side: c4_ok; gemm_c4.h the kernel, gemm_shortk.h what it shares with k_gemm_c8 / k_gemm_ar)
#include "gemm_c4.h"
static int g_c4_chunk = getenv("TF_C4_CHUNK") ? atoi(getenv("TF_C4_CHUNK")) : 0;   // A/B: tiles per chunk of k_gemm_c4's walk (0 = per-shape choice)
int TFK(tfk_launch_c4)(const GemmP& p, hipStream_t st) {
  constexpr int smem = 2 * (128 + 128) * 128 + 4 * 64 * 8;   // the two-slot ring (the epilogue's patches live in slot 1) + the LayerNorm row-sum exchange
  static bool attr_set = false;
  if (int e = shortk_set_lds(attr_set, smem, {(const void*)k_gemm_c4<false, kBF>, (const void*)k_gemm_c4<true, kBF>})) return e;
  const int tiles = p.ntm * p.ntn;
  GemmP q = p;
  q.c4_chunk = g_c4_chunk > 0 ? g_c4_chunk : shortk_chunk(p, tiles, 8);
  const int chunks = (tiles + q.c4_chunk - 1) / q.c4_chunk;
  const int grid = chunks < 2 * shortk_num_cus() ? chunks : 2 * shortk_num_cus();   // two resident blocks per CU walk the tile list
  if (p.ln_colsum) hipLaunchKernelGGL((k_gemm_c4<true, kBF>), dim3(grid), dim3(256), smem, st, q);
  else hipLaunchKernelGGL((k_gemm_c4<false, kBF>), dim3(grid), dim3(256), smem, st, q);
  TF_LAUNCH_CHECK();
  return TF_OK;
}
