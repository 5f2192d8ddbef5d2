// Part of the implicit-GEMM family of csrc/gemm.hip (see its head comment).
// What the three LDS-DMA RING kernels have in common -- k_igemm (gemm_igemm.h), its patch form k_igemm_patch (gemm_patch.h) and the e4m3 form
// k_igemm8 (gemm_igemm8.h) -- and can share without compiling to another schedule, each piece ONCE:
//   the head of a block (roles, tile, K range); the lane -> source chunk map and the weight-row offset of the staging (all four sites); the barrier;
//   the diagnostics of k_igemm's tagged builds (gemm_stamp.h).
// What is NOT here stays in the kernels: the staging geometry of the activation rows, the (tap, channel) walk, the loader and consumer K loops and the
// exit sequence (one ring_exit for both roles was built and MEASURED: K loops of WIDE instances +1 ... 3 instructions, 512 x 1280 x 1280 0.7 % slower).  Written as shared functions taking functors they compiled every instance to another instruction stream (other block layout, other
// register allocation, +-1 ... 4 instructions per K tile in some instances: profiles/ring_refactor_resources.txt), and the K loop's schedule is not to move.
// Scalars travel BY VALUE: a RingBlock handed on by const reference cost the epilogue behind it the known bits of `lane` (signed divisions came back).
#pragma once
#include "gemm_common.h"
#include "gemm_stamp.h"

__device__ __forceinline__ void ring_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- the head of a block -------------------------------------------------------------------------------------------------------------------------
// 8 waves: 0-3 consumers, 4-7 loaders, w4 = the wave's index inside its role; the block's tile (m0, n0) and its K tiles [kt_begin, kt_end) of split `split`
struct RingBlock {
  int lane, wid, w4, split, m0, n0, kt_begin, kt_end, nt;
  bool loader;
};
template <int BM, int BN>
__device__ __forceinline__ RingBlock ring_block(const GemmP& p) {
  RingBlock b;
  const int tid = threadIdx.x;
  b.lane = tid & 63;
  b.wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  b.loader = b.wid >= 4;
  b.w4 = b.wid & 3;
  const int ntiles = p.ntm * p.ntn;
  const int nblk = ntiles * p.splitk;
  const int bid = xcd_order(blockIdx.x, nblk);
  b.split = bid / ntiles;
  const TileMN tmn = tile_decode(bid - b.split * ntiles, p.order, p.ntm, p.ntn);
  b.m0 = tmn.m * BM; b.n0 = tmn.n * BN;
  b.kt_begin = b.split * p.ktiles_per_split;
  b.kt_end = min(p.ktiles, b.kt_begin + p.ktiles_per_split);
  b.nt = b.kt_end - b.kt_begin;
  return b;
}

// ---- staging, 128-byte rows (fp16 / bf16) --------------------------------------------------------------------------------------------------------
// A 1-KiB piece is 8 rows, lane -> row lane >> 3 of its piece, LDS chunk lane & 7.  The XOR swizzle is applied on the SOURCE chunk (the LDS image stays
// lane-linear): chunk ^ ((row >> 1) & 7); a wave's pieces are g = w4 (mod 4), so the term is a per-thread constant.
__device__ __forceinline__ int ring_src_chunk128(int lane, int w4) { return (lane & 7) ^ ((4 * (w4 & 1) + (lane >> 4)) & 7); }
// byte offset of this lane's 16 bytes of K tile 0 in weight row n (16-byte chunk `chunk`; ES bytes per element) ...
template <int ES>
__device__ __forceinline__ unsigned ring_weight_off(const GemmP& p, int n, int chunk) {
  return (unsigned)(n * p.K + chunk * (16 / ES)) * (unsigned)ES;
}
// ... and TF_OOB beyond N.  (The loaders of k_igemm / k_igemm8 keep their own `if (n < p.N)` around ring_weight_off: their rows start out as TF_OOB, and
// the select in place of the guarded store moved k_igemm's WIDE consumer loops by 1 ... 3 instructions.)
template <int ES>
__device__ __forceinline__ unsigned ring_weight_row(const GemmP& p, int n, int chunk) {
  return n < p.N ? ring_weight_off<ES>(p, n, chunk) : TF_OOB;
}
