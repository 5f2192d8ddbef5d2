// Part of the implicit-GEMM family of csrc/gemm.hip (see its head comment).
// The diagnostics of k_igemm's tagged builds, kept out of the kernel's text: the kernel calls these methods unconditionally and in the shipped
// library (TF_IGEMM_STAMP == 0) every one of them is empty.
//   -DTF_IGEMM_STAMP=1 (tools/igemm_stamp.py): wave 0 (a consumer) and wave 4 (a loader) of every block keep four stamps of the constant 100 MHz
//     clock each and store them when they leave, 8 words per block: [0] entry [1] K loop done (behind barrier X) [2] epilogue stores issued
//     [3] stores drained | [4] entry [5] K tile 0 landed [6] last stage issued [7] left.  The fences idle nothing the shipped kernel overlaps
//     across these points (they sit at barriers).
//   -DTF_IGEMM_STAMP=2 (tools/igemm_loop_stamp.py): additionally per-K-tile stamps (s_memtime, core clock) of block 0's wave 4 (loader: 0 top,
//     1 tile it + 1 landed, 2 behind barrier(it), 3 next stage issued) and wave 0 (consumer: 4 fragments of tile it in registers, 5 behind
//     barrier(it)) for K tiles 4 .. 4 + 255, kept in the LDS above the ring (the launch gets all 160 KiB) and copied out behind the per-block
//     table (256 x 8 words) when the waves leave.  Only where lgkmcnt is 0 anyway, so no overlap of the shipped loop is fenced off.
#pragma once
#include "gemm_common.h"

#if TF_IGEMM_STAMP
struct RingStamps {
  unsigned long long t[4];
  unsigned long long* out;
  unsigned lp_base;
  int lane, wid;
  bool lp_on;
  // `deep`: the deep ring with the A/B consumer loop (the only form whose K loop is stamped per tile)
  __device__ __forceinline__ void init(const GemmP& p, const char* smem, int lane_, int wid_, bool deep) {
    t[0] = __builtin_amdgcn_s_memrealtime(); t[1] = t[2] = t[3] = 0;
    out = p.stamp; lane = lane_; wid = wid_;
    lp_on = TF_IGEMM_STAMP == 2 && blockIdx.x == 0 && lane == 0 && (wid == 0 || wid == 4) && p.stamp && deep;
    lp_base = lds_off(smem) + 163840u - 256u * 32u;
  }
  __device__ __forceinline__ void mark(int k) {
    __builtin_amdgcn_sched_barrier(0); t[k] = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
  __device__ __forceinline__ void loop(int it, int k) const {
    if (TF_IGEMM_STAMP != 2 || !lp_on || it < 4 || it >= 260) return;
    unsigned long long t_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory");
    asm volatile("ds_write_b32 %0, %1" :: "v"(lp_base + (unsigned)((it - 4) * 8 + k) * 4u), "v"((unsigned)t_) : "memory");
  }
  // wave `w` (0 or 4) stores its four stamps at words [w, w + 4) of its block's row, then block 0 copies its columns of the loop table out
  __device__ __forceinline__ void leave(int w) {
    if (wid == w && out && lane == 0 && blockIdx.x < 8192) { unsigned long long* d = out + (size_t)blockIdx.x * 8 + w; d[0] = t[0]; d[1] = t[1]; d[2] = t[2]; d[3] = t[3]; }
    if (TF_IGEMM_STAMP != 2 || !lp_on) return;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int i = 0; i < 256 * 8; ++i) {
      if (((i & 7) < 4) != (wid == 4)) continue;           // each wave copies its own columns
      unsigned v_;
      asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v_) : "v"(lp_base + (unsigned)i * 4u) : "memory");
      reinterpret_cast<unsigned*>(out + 8192 * 8)[i] = v_;
    }
  }
};
#else
struct RingStamps {
  __device__ __forceinline__ void loop(int, int) const {}
  __device__ __forceinline__ void init(const GemmP&, const char*, int, int, bool) {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void drain() {}
  __device__ __forceinline__ void leave(int) {}
};
#endif
