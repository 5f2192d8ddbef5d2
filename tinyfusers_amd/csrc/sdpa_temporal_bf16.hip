// bfloat16 twin of the temporal attention kernel (sdpa_temporal.hip)
#define TF_TU_BF 1
#include "sdpa_temporal.hip"
