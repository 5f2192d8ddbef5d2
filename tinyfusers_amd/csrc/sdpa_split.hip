// key-slice instances of the LDS-DMA attention kernel (k_sdpa_split: sdpa_dma_body<..., KS = 2, SR>), in a translation unit of their own: the code objects of sdpa.hip stay what they were without them
#define TF_TU_SPLIT 1
#include "sdpa.hip"
