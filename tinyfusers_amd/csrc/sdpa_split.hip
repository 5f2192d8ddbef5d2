// Key-slice instances of the LDS-DMA attention kernel (k_sdpa_split: sdpa_dma_body.inc with KS = 2), in a translation unit of their own: the code objects of
// sdpa.hip stay what they were without them.  sdpa.hip's rule picks a form (SDPA_SPLIT_*, sdpa_common.h); tfk_sdpa_split launches it.
//
// KS > 1: key slices inside the block, for grids that leave the SIMDs short of waves when every (batch, head, query) is
// already spent.  The NW waves are NQ = NW / KS query groups x KS slices; slice s walks the contiguous key tiles [s TPS, (s + 1) TPS), TPS =
// ceil(ntiles / KS) (the last slice shorter or empty), through a ring of its own (SR stages, staged by its own NQ waves), with its own online softmax
// ("first tile adopts its maximum" per slice).  EVERY wave runs TPS loop iterations and executes the s_barrier of each: a slice that has run out of
// tiles has nothing in flight (vmcnt(0) is immediate), issues nothing and skips the work behind the barrier, never the barrier.  After the loop the
// rings are dead: the slices >= 1 leave their unnormalised O^T, row sums and reference maxima in that LDS and the slice-0 waves fold them in in slice
// order, O = sum_s O_s 2^(m_s - M), M = max m_s over the slices that saw a tile (an empty slice contributes nothing; a weight that underflows to 0 is
// what it should be) -- no atomics, no traffic between blocks, the same sum in the same order on every run.
#include "sdpa_common.h"

template <int HS, int QT, int NW, int KS, int SR, bool BF>
__global__ void __launch_bounds__(NW * 64) k_sdpa_split(const SdpaP p) {
  constexpr int DBG = 0;
#include "sdpa_dma_body.inc"
}

template <int HS, int QT, int NW, int KS, int SR>
static int launch_sdpa_split(const SdpaP& p, hipStream_t st) {
  constexpr int smem = KS * SR * SdpaDma<HS>::STAGE_B;
  static_assert(smem <= 160 * 1024, "the rings must fit the CU's LDS");
  return launch_sdpa_kernel<k_sdpa_split<HS, QT, NW, KS, SR, kBF>>(p, p, smem, 16 * (NW / KS) * QT, NW, st);
}

int TFK(tfk_sdpa_split)(const SdpaP& p, int form, hipStream_t st) {
  if (form == SDPA_SPLIT_40_W16) return launch_sdpa_split<40, 2, 16, 2, 4>(p, st);
  if (form == SDPA_SPLIT_80_Q16) return launch_sdpa_split<80, 1, 8, 2, 3>(p, st);
  tf_set_error("tf_sdpa: no split kernel of form %d", form);
  return TF_E_UNSUPPORTED;
}
