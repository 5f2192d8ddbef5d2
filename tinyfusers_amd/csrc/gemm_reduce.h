// The split-K reduce launches (gemm_reduce.hip) as the dispatcher sees them.  Host side only: no kernel translation unit includes this.
#pragma once
#include "gemm_common.h"

// The launch that finishes a GEMM whose K range was split (p.splitk > 1; nothing to do otherwise): partials summed in split order + bias + bias_nc +
// residual -> y; with p.gn_part also the GroupNorm statistics of y, and with p.on_z (where tfk_splitk_reduce_applies_gn) the normalised z in
// the same launch.  *p.on_applied tells the caller whether z was written.
int tfk_launch_splitk_reduce(const GemmP& p, hipStream_t st);
// does that launch, for outputs of HoWo pixels x N channels in G groups, normalise as well (k_splitk_reduce_gn_apply)?
bool tfk_splitk_reduce_applies_gn(int HoWo, int N, int G);
