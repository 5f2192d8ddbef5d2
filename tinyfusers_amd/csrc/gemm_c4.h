// Part of the implicit-GEMM family of csrc/gemm.hip (see its head comment); split into translation units so that the
// instances compile in parallel.
#pragma once
#include "gemm_shortk.h"

// =====================================================================================================================
// SHORT-K kernel (round 3): Linear / 1x1 convolution with K <= a few K tiles and many output tiles -- q|k|v, to_out, GEGLU projection
// (ff/linear.py:112-121, ff/nn.py:5-12, attention/attention.py:35-41 of the reference).  For these shapes every part of a launch of the
// kernels above is near a bound of its own -- block dispatch + prologue ~3.4 us per round of blocks, operand re-reads from L2, the MFMAs,
// the output stores at the HBM write rate -- but the parts run one AFTER the other (tools/geglu_dbg.py: 8.5 + 10 + 9 + 5 ~ 31.6 us for
// 8192 x 2560 x 320, where max() would be 10): a block is a serial chain and a CU holds two of them.  This kernel removes the seams:
//   * PERSISTENT: 2 blocks of 4 waves per CU for the whole launch, each walking its own list of 128 x 128 tiles -- no dispatch or argument
//     loads per tile, and the stores of tile i drain while tile i + 1 loads and multiplies (nothing ever waits for a store);
//   * all four waves load and compute (2 x 2 wave tiles of 64 x 64); 2-slot LDS-DMA ring, one s_barrier per K tile; the first K tile of
//     the NEXT output tile is issued before the epilogue of this one (cross-tile prefetch: the ring slot it lands in is not the one the
//     epilogue borrows);
//   * epilogue without a block barrier: LayerNorm fold / bias / GEGLU in registers on the accumulators (a lane owns 4 consecutive channels of
//     a pixel), rounded to fp16, transposed through a PRIVATE per-wave LDS patch (half a wave tile at a time) into 16-byte row segments,
//     residual added there, stored;
//   * the two blocks of a CU are independent programs: one's epilogue and first-tile latency overlap the other's MFMAs.
// S = 1 / stride 1 / no padding (rows are contiguous K vectors; the concat pair of the FF2 . proj_out fold is two sources), channel
// counts on the 64 grid, fp16, no split-K / statistics / time embedding (those launches keep the kernels above).
// This file: the two-slot ring protocol (barriers, the counted wait in front of a tile's first K tile) and the kernel's place in LDS.  The tile walk, the
// staging, the K step, the bias request, the LayerNorm fold and the transposing store are gemm_shortk.h's, shared with k_gemm_c8 and k_gemm_ar.
template <bool LNF, bool BF = false>   // BF: bfloat16 operands / outputs (gemm_k_c4_bf16.hip)
__global__ void __launch_bounds__(256, 2) k_gemm_c4(const GemmP p) {
  constexpr int BM = 128, BN = 128, MJ = 4, NI = 4;
  constexpr int STAGE = (BM + BN) * 128;                  // 32 KiB
  constexpr int PATCH = 32 * 144;                         // per-wave transpose patch: 32 rows x (128 + 16) bytes
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid & 1, wn = wid >> 1;
  const int lg = lane >> 4;
  const unsigned lds0 = lds_off(smem);
  const int ntm = p.ntm, ntn = p.ntn, ntiles = ntm * ntn;
  const int nt = p.ktiles;
  const int gstep = gridDim.x;
  const int M_ = p.M, N_ = p.N;
  const int fo = sk_frag_off(lane);
  const int xo = wm * 64 * 128 + fo, wo_ = (BM + wn * 64) * 128 + fo;
  char* const patch = smem + STAGE + wid * PATCH;         // inside ring slot 1 (the next tile's first K tile lands in slot 0)
  f2* const stats = reinterpret_cast<f2*>(smem + 2 * STAGE);   // [4 waves][64 rows] halves of the LayerNorm row sums (behind the ring)

  // all four waves stage: activation pieces wid + 4 i (i < 4), weight pieces likewise -- 8 LDS-DMA pieces per wave and K tile
  SkStager<4, 4, 4> sg(p, wid, lane);
  auto setup = [&](int tile, int& m0, int& n0) {
    const TileMN t = tile_decode(tile, p.order, ntm, ntn);
    m0 = t.m * BM; n0 = t.n * BN;
    sg.rows_a(m0); sg.rows_w(n0);
  };
  auto stage = [&](int slot, int kt) {                    // K tile kt of the tile whose rows are in sg
    const unsigned base = lds0 + (unsigned)slot * STAGE;
    sg.stage_a(kt, base); sg.stage_w(kt, base + (unsigned)(BM * 128));
  };
  auto barrier = [&]() {
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  const int chunk = p.c4_chunk;                           // the chunked walk: sk_next_tile
  int cq_ = blockIdx.x, ce_ = 0;                          // chunk index, tile inside the chunk
  int tile = cq_ * chunk;
  if (tile >= ntiles) return;
  int m0, n0;
  setup(tile, m0, n0);
  stage(0, 0);
  float ln_mean[MJ], ln_rstd[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) { ln_mean[j] = 0.f; ln_rstd[j] = 0.f; }
  int stat_m0 = -1;
  int pend = 0;                                           // stores issued behind the prefetch of this tile's K tile 0 (0: unknown -> full wait)
  while (tile >= 0) {
    const bool need_stats = LNF && m0 != stat_m0;
    f4 acc[NI][MJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
    float ls[MJ], lq[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) { ls[j] = 0.f; lq[j] = 0.f; }
    h4 braw[NI];
    f4 cq[NI];
    sk_request<LNF>(p, n0 + wn * 64, lg, braw, cq);
    const int young = pend > 0 ? pend + (p.bias ? NI : 0) + (LNF ? NI : 0) : 0;
    // ---- K loop: tile t in slot t & 1, one barrier per K tile, one K tile in flight
    for (int t = 0; t < nt; ++t) {
      // K tile t has landed.  For t = 0 it was issued in front of the previous tile's epilogue: where that epilogue's vector-memory
      // instructions are known to be `pend` stores, followed by this tile's bias / column-sum loads and nothing else, those `young`
      // ones stay in flight (the counter retires in issue order)
      if (t == 0) {
        if (young == 4) wait_vm<4>();
        else if (young == 8) wait_vm<8>();
        else if (young == 12) wait_vm<12>();
        else if (young == 16) wait_vm<16>();
        else wait_vm<0>();
      }
      else wait_vm<0>();
      barrier();
      if (t + 1 < nt) stage((t + 1) & 1, t + 1);
      const char* sb = smem + (t & 1) * STAGE;
      h8 wf[2][NI], xf[2][MJ];
#pragma unroll
      for (int f = 0; f < 2; ++f) { sk_read_half(xf[f], sb, xo, f); sk_read_half(wf[f], sb, wo_, f); }
      wait_lds_reads();
      __builtin_amdgcn_sched_barrier(0);
      if (LNF && need_stats) {
        // row statistics from the fragments: the two waves that share these 64 rows (wn = 0, 1) take one 32-deep k-step each
        if (wn == 0) sk_stats_half<BF>(xf[0], ls, lq); else sk_stats_half<BF>(xf[1], ls, lq);
      }
#pragma unroll
      for (int f = 0; f < 2; ++f) sk_mma_half<BF>(wf[f], xf[f], acc);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (LNF && need_stats) sk_rowsum_put(stats, wid, lane, ls, lq);   // the partner's half comes back behind the barrier
    barrier();                                             // every wave is done with the ring
    // ---- LayerNorm fold and bias on the accumulators (registers)
    sk_request_pin<LNF>(braw, cq);
    if constexpr (LNF) {
      if (need_stats) { sk_rowsum_get(stats, wid ^ 2, lane, ls, lq, p.K, p.ln_eps, ln_mean, ln_rstd); stat_m0 = m0; }
    }
    sk_fold<LNF, BF>(acc, ln_mean, ln_rstd, cq, braw);
    asm volatile("" ::: "memory");
    // ---- the next tile's rows and its first K tile (slot 0), in flight during the rest of this tile's epilogue
    const int cm0 = m0, cn0 = n0;
    const int next = sk_next_tile(cq_, ce_, chunk, gstep, ntiles);
    if (next >= 0) { setup(next, m0, n0); stage(0, 0); }
    pend = (cm0 + BM <= M_ && cn0 + BN <= N_ && !p.residual) ? sk_wave_tile_stores(p.act == 1) : 0;
    sk_store_wave_tile<LNF, BF>(p, acc, lds_off(patch), cm0 + wm * 64, cn0 + wn * 64, lane);
    tile = next;
  }
}
