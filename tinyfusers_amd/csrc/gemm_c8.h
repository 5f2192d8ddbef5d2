// Part of the implicit-GEMM family of csrc/gemm.hip (see its head comment); split into translation units so that the
// instances compile in parallel.
#pragma once
#include "gemm_shortk.h"

// =====================================================================================================================
// k_gemm_c8 (round 5): the WIDE form of the persistent short-K kernel k_gemm_c4 for launches that fill the chip with 256-row tiles --
// BASELINE config 5's linears and 1 x 1 convolutions with K <= 6400 (ff/linear.py:112-121, ff/nn.py:5-23, attention/attention.py:35-41 of the
// reference): q|k|v, to_out, the GEGLU projection, FF2, proj_in / proj_out.  Those were the largest block of config 5's GEMM time (7.05 of 15.1 ms at
// 0.35-0.88 PFLOP/s, profiles/r04_gemm_shapes_images4_latent96_fp16.txt) on two kernels that each lacked half of what the shapes need: k_gemm_c4 has the
// register epilogue and the cross-tile prefetch but 128 x 128 tiles (64 FLOP per ingested byte) and ONE 32-KiB K tile in flight per block; the ping-pong
// kernel has the 256-row tile but a shared-scratch epilogue with two block barriers per half and no overlap across tiles.  This kernel is both:
//   * ONE block of 8 waves per CU for the whole launch, walking its list of 256 x 128 tiles (4 x 2 wave tiles of 64 x 64: k_gemm_c4's fragment code);
//     85 FLOP per ingested byte, a third more than the 128 x 128 tile;
//   * a THREE-slot LDS-DMA ring of 48-KiB K tiles that runs straight across tile boundaries (slot = running K-tile index mod 3): two K tiles in
//     flight at any time, and the first TWO K tiles of the next output tile are issued before this tile's epilogue starts;
//   * k_gemm_c4's epilogue: LayerNorm fold / bias / GEGLU on the accumulators in registers, transposed half a wave tile at a time through a private
//     per-wave LDS patch -- in the ring slot the next two K tiles do not land in -- residual added on the row side, 16-byte stores that nothing waits
//     for (counted vmcnt in front of the next tile's K tiles).
// Eligibility = k_gemm_c4's (c4_ok: 1 x 1 / stride 1, channel counts on the 64 grid, no split-K / statistics / time embedding).
// This file: the three-slot ring across tiles (slots, barriers, the counted vmcnt chains) and the kernel's place in LDS.  The tile walk, the staging, the K step,
// the bias request, the LayerNorm fold and the transposing store are gemm_shortk.h's, shared with k_gemm_c4 and k_gemm_ar.
template <bool LNF, bool BF = false>
__global__ void __launch_bounds__(512, 2) k_gemm_c8(const GemmP p) {
  constexpr int BM = 256, BN = 128, MJ = 4, NI = 4;
  constexpr int STAGE = (BM + BN) * 128;                  // 48 KiB
  constexpr int PATCH = 32 * 144;                         // per-wave transpose patch: 32 rows x (128 + 16) bytes
  constexpr int LPT = 6;                                   // LDS-DMA pieces per wave and K tile: 4 activation + 2 weight
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid & 3, wn = wid >> 2;                   // 4 (rows) x 2 (columns) wave tiles of 64 x 64
  const int lg = lane >> 4;
  const unsigned lds0 = lds_off(smem);
  const int ntm = p.ntm, ntn = p.ntn, ntiles = ntm * ntn;
  const int nt = p.ktiles;
  const int gstep = gridDim.x;
  const int M_ = p.M, N_ = p.N;
  const int fo = sk_frag_off(lane);
  const int xo = wm * 64 * 128 + fo, wo_ = (BM + wn * 64) * 128 + fo;
  f2* const stats = reinterpret_cast<f2*>(smem + 3 * STAGE);   // [8 waves][64 rows] halves of the LayerNorm row sums (behind the ring)

  // all eight waves stage: activation pieces wid + 8 i (i < 4), weight pieces wid + 8 i (i < 2) -- LPT pieces per wave and K tile
  SkStager<8, 4, 2> sg(p, wid, lane);
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
  int s0 = 0;                                             // ring slot of this tile's K tile 0 (the ring runs across tiles: slot = (s0 + t) % 3)
  stage(0, 0);
  if (nt > 1) stage(1, 1);
  float ln_mean[MJ], ln_rstd[MJ];
#pragma unroll
  for (int j = 0; j < MJ; ++j) { ln_mean[j] = 0.f; ln_rstd[j] = 0.f; }
  int stat_m0 = -1;
  int pend = -1;                                          // vector-memory instructions of the previous epilogue behind this tile's prefetched K tiles (-1: unknown -> full wait)
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
    // what is younger than this tile's K tile 0 in the wave's vector-memory queue: K tile 1 (LPT, if any), the previous epilogue's stores (pend), these loads
    const int nload = (p.bias ? NI : 0) + (LNF ? NI : 0);
    const int young0 = pend >= 0 ? (nt > 1 ? LPT : 0) + pend + nload : -1;
    // ---- K loop: K tile t in slot (s0 + t) % 3; at the top of step t tile t must have landed (tile t + 1 may be in flight); the barrier then frees
    // the slot of tile t - 1 for tile t + 2
    int sl = s0;                                           // slot of K tile t
    for (int t = 0; t < nt; ++t) {
      if (t == 0) {
        if (young0 == 6) wait_vm<6>(); else if (young0 == 10) wait_vm<10>(); else if (young0 == 14) wait_vm<14>(); else if (young0 == 18) wait_vm<18>();
        else if (young0 == 22) wait_vm<22>(); else if (young0 == 4) wait_vm<4>(); else if (young0 == 8) wait_vm<8>(); else if (young0 == 12) wait_vm<12>();
        else if (young0 == 16) wait_vm<16>(); else wait_vm<0>();
      } else if (t == 1) {
        // K tile 1 was issued in front of the previous epilogue too: younger than it are that epilogue's stores, this tile's bias loads and K tile 2
        const int y1 = pend >= 0 ? pend + nload + (nt > 2 ? LPT : 0) : -1;
        if (y1 == 6) wait_vm<6>(); else if (y1 == 10) wait_vm<10>(); else if (y1 == 14) wait_vm<14>(); else if (y1 == 18) wait_vm<18>(); else if (y1 == 22) wait_vm<22>();
        else if (y1 == 4) wait_vm<4>(); else if (y1 == 8) wait_vm<8>(); else if (y1 == 12) wait_vm<12>(); else if (y1 == 16) wait_vm<16>(); else wait_vm<0>();
      } else {
        if (t + 1 < nt) wait_vm<LPT>(); else wait_vm<0>();   // tile t landed, tile t + 1 in flight (everything else in the queue is older than tile t)
      }
      barrier();
      if (t + 2 < nt) { int s2 = sl + 2; s2 = s2 >= 3 ? s2 - 3 : s2; stage(s2, t + 2); }
      const char* sb = smem + sl * STAGE;
      sl = sl == 2 ? 0 : sl + 1;
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
    barrier();                                             // every wave is done with the ring (all three slots are free)
    // ---- LayerNorm fold and bias on the accumulators (registers)
    sk_request_pin<LNF>(braw, cq);
    if constexpr (LNF) {
      if (need_stats) { sk_rowsum_get(stats, wid ^ 4, lane, ls, lq, p.K, p.ln_eps, ln_mean, ln_rstd); stat_m0 = m0; }   // the partner along n: same rows, the other k-step
    }
    sk_fold<LNF, BF>(acc, ln_mean, ln_rstd, cq, braw);
    asm volatile("" ::: "memory");
    // ---- the next tile's rows and its first TWO K tiles, in flight during this tile's epilogue: they land in slots s1, s1 + 1 (s1 = the slot behind this
    // tile's last K tile); the epilogue's patches live in the third slot -- the one this tile's LAST K tile occupied, free since the barrier above
    const int cm0 = m0, cn0 = n0;
    int s1 = s0 + nt % 3; s1 = s1 >= 3 ? s1 - 3 : s1;
    int sp = s1 + 2; sp = sp >= 3 ? sp - 3 : sp;            // = slot of K tile nt - 1
    const int next = sk_next_tile(cq_, ce_, chunk, gstep, ntiles);
    if (next >= 0) {
      setup(next, m0, n0);
      stage(s1, 0);
      if (nt > 1) { int s11 = s1 + 1; s11 = s11 >= 3 ? s11 - 3 : s11; stage(s11, 1); }
    }
    s0 = s1;
    pend = (cm0 + BM <= M_ && cn0 + BN <= N_ && !p.residual) ? sk_wave_tile_stores(p.act == 1) : -1;
    sk_store_wave_tile<LNF, BF>(p, acc, lds_off(smem + sp * STAGE + wid * PATCH), cm0 + wm * 64, cn0 + wn * 64, lane);
    tile = next;
  }
}
