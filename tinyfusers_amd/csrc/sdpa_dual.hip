// dual (two key sets, decoupled cross-attention) instances of the LDS-DMA attention kernel (k_sdpa_dual: sdpa_dma_body.inc with TF_SDPA_BODY_DUAL) and tf_sdpa_dual_16, in a translation unit of their own: the code objects of sdpa.hip / sdpa_split.hip stay what they were without them
#define TF_TU_DUAL 1
#include "sdpa.hip"
