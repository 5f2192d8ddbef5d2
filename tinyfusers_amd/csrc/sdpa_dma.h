// k_sdpa_dma: the LDS-DMA attention kernel (layouts and ring: sdpa_common.h; the body: sdpa_dma_body.inc, one text shared with k_sdpa_split, k_sdpa_dual and
// k_sdpa_pag) and its launcher, which in the ablation library also holds the dispatch onto the ablation instances.
#pragma once
#include "sdpa_common.h"

// NW = waves per block (4, or 8 for long sequences: twice the queries per fetched K/V tile -- the tile fetch, not the barrier, is what the
// ablation prices at 19 % of the d = 40 loop at 9216 tokens -- and four waves per SIMD instead of three at two blocks per CU)
template <int HS, int QT, int DBG = 0, int NW = 4, bool BF = false>        // DBG: compile-time ablation mask (tools/sdpa_dbg.py; bits as SdpaP::dbg); BF: bfloat16 q / k / v / o (sdpa_bf16.hip)
__global__ void __launch_bounds__(NW * 64) k_sdpa_dma(const SdpaP p) {
  constexpr int KS = 1, SR = 0;      // no key slices: the kernel as it always was
#include "sdpa_dma_body.inc"
}

template <int HS, int QT, int NW = 4>
static int launch_sdpa_dma(const SdpaP& p, hipStream_t st) {
  constexpr int smem = sdpa_ring_bytes<HS, NW>(), QB = 16 * NW * QT;
#if defined(TF_ABLATION) && !TF_TU_BF   // the ablation library only (python -m tinyfusers_amd.build --ablation; tools/sdpa_dbg.py): wrong results by design
  if constexpr (HS == 40 && QT == 2 && NW == 4) {
    if (p.dbg) {
      const dim3 grid((unsigned)((p.Tq + QB - 1) / QB * p.NH * p.B));
      switch (p.dbg) {
#define TF_SDPA_DBG_CASE(M) case M: hipLaunchKernelGGL((k_sdpa_dma<HS, QT, M>), grid, dim3(256), smem, st, p); break;
        TF_SDPA_DBG_CASE(1) TF_SDPA_DBG_CASE(64) TF_SDPA_DBG_CASE(65) TF_SDPA_DBG_CASE(2) TF_SDPA_DBG_CASE(4) TF_SDPA_DBG_CASE(6) TF_SDPA_DBG_CASE(32)
        TF_SDPA_DBG_CASE(34) TF_SDPA_DBG_CASE(8) TF_SDPA_DBG_CASE(16) TF_SDPA_DBG_CASE(24) TF_SDPA_DBG_CASE(62) TF_SDPA_DBG_CASE(89) TF_SDPA_DBG_CASE(128)
#undef TF_SDPA_DBG_CASE
        default: tf_set_error("tf_sdpa_f16: no ablation build for TF_SDPA_DBG=%d", p.dbg); return TF_E_UNSUPPORTED;
      }
      TF_LAUNCH_CHECK();
      return TF_OK;
    }
  }
#endif
  return launch_sdpa_kernel<k_sdpa_dma<HS, QT, 0, NW, kBF>>(p, p, smem, QB, NW, st);
}
