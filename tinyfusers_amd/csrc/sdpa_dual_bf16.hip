// bfloat16 twins of the dual attention instances the launcher routes to (sdpa_dual.hip)
#define TF_TU_BF 1
#define TF_TU_DUAL 1
#include "sdpa.hip"
