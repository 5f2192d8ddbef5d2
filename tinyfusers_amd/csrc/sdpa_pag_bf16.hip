// bfloat16 twins of the perturbed-attention instances the launcher routes to (sdpa_pag.hip)
#define TF_TU_BF 1
#include "sdpa_pag.hip"
