// bfloat16 twins of the dual attention instances the launcher routes to (sdpa_dual.hip)
#define TF_TU_BF 1
#include "sdpa_dual.hip"
