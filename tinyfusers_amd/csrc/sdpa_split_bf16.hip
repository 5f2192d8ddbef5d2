// bfloat16 twins of the key-slice attention instances the launcher routes to (sdpa_split.hip)
#define TF_TU_BF 1
#include "sdpa_split.hip"
