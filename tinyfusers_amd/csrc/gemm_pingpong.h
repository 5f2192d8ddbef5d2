// Part of the implicit-GEMM family of csrc/gemm.hip (see its head comment).
// What the two ping-pong kernels have in common -- k_igemm_pp (gemm_pp.h) and its patch form k_igemm_pp3 (gemm_pp3.h) -- each piece ONCE:
//   the LDS layout (ring, scale tables, the epilogue's share) that kernel AND launcher read; the weight rows of a wave and the LDS-DMA of their pieces;
//   the SGPR descriptor of an activation source and of its scale bytes; the lean-addressing pixel index and tap mask; the MFMA block of a phase;
//   the per-channel weight scales of the e4m3 form; the bias / time-embedding prefetch and the two-pass epilogue; the barrier.
// What is NOT here is what differs: the ring protocol of each kernel (which wave issues which load in which phase, the counted vmcnt waits, the
// barriers), the activation gather (tiles per tap / one patch per slab) and the fragment addressing.
// The counted waits of the kernels rest on the instruction counts of these pieces: pp_stage_weights issues WPW LDS-DMA pieces (one fewer on waves
// >= WREM where BN / 8 is no multiple of 8) and returns that number; nothing else in this file issues a vector-memory load inside a K loop.
#pragma once
#include "gemm_common.h"

// ---- LDS layout ------------------------------------------------------------------------------------------------------------------------------------
// The epilogue's share (it re-uses the ring's LDS behind the last barrier of the K loop), two passes of BM / 2 rows: the 2 x 2-wave-tile scratch of
// igemm_scratch_write<BM / 2, BN> | LayerNorm (mean, rstd) of the pass's rows | GroupNorm statistics table | bias / time-embedding table (3 x BN floats)
template <int BM, int BN>
struct PpEpiLds {
  static constexpr int BS = BM / 2;                                       // rows of an epilogue pass
  static constexpr int scratch = 4 * (BS / 2) * (BN / 2 + 4) * 4;
  static constexpr int ln_stats = scratch;                                // byte offsets of the tables behind the scratch
  static constexpr int lbt = scratch + BS * 8 + 4 * BN * 8;
  static constexpr int epilogue = lbt + 3 * BN * 4;
};
// k_igemm_pp: NS ring slots of (BM + BN) x 128 B | F8: NS scale tables (one dword per row and scale load, 4 waves x 64 rows)
template <int BM, int BN, bool F8, bool H2>
struct PpLds : PpEpiLds<BM, BN> {
  static constexpr int STAGE = (BM + BN) * 128;
  static constexpr int NS = (163840 / STAGE) >= 3 ? 3 : 2;
  static constexpr int SCL = F8 ? (H2 ? 2 : 1) : 0;                       // scale loads per K tile of a wave that stages scales (waves 4-7)
  static constexpr int SCS = SCL * 1024;                                  // bytes of a slot's scale table (the 192-row tile leaves the last 64 rows unused)
  static constexpr int scales = NS * STAGE;                               // byte offset of the scale tables
  static constexpr int ring = scales + NS * SCS;
  static constexpr int total = ring > PpEpiLds<BM, BN>::epilogue ? ring : PpEpiLds<BM, BN>::epilogue;
};
// k_igemm_pp3: patch buffer 0 | patch buffer 1 | NS weight slots | F8: two scale patches; fp16: slot 1 of the extra segment where a patch buffer is too small for two
template <int BN, int W, bool F8, bool H2>
struct Pp3Lds : PpEpiLds<192, BN> {
  static constexpr int BM = 192, NS = 3;
  static constexpr int WST = BN * 128;                                    // bytes of a weight ring slot
  static constexpr int PW = W + 4, PROWS = (BM / W + 2) * PW, NPP = (PROWS + 7) / 8, PB = NPP * 1024;     // patch: row pitch, rows, 8-row pieces, bytes of a buffer
  static constexpr int NSW = (PROWS + 63) / 64;                           // waves that fetch scales
  static constexpr int SCT = F8 ? NSW * 256 : 0;                          // bytes of a scale table: one dword per patch row, whole 64-row wave loads
  static constexpr int SCB = (H2 ? 2 : 1) * SCT;                          // bytes of a scale patch (H2: two tables)
  static constexpr int AST = BM * 128;                                    // bytes of an activation tile of the extra 1x1 segment
  static constexpr int XS1 = 2 * AST <= PB ? AST : -1;                    // its slot 1: behind slot 0 in the free patch buffer, or (-1) in the spare LDS behind the weight ring
  static constexpr int weights = 2 * PB;                                  // byte offsets
  static constexpr int spare = weights + NS * WST;                        // scale patches / slot 1 of the extra segment
  static constexpr int ring = spare + (F8 ? 2 * SCB : XS1 > 0 ? 0 : AST);
  static constexpr int total = ring > PpEpiLds<192, BN>::epilogue ? ring : PpEpiLds<192, BN>::epilogue;
};
// the dynamic LDS of shipped instances, as it was when every kernel and launcher did this arithmetic on its own
static_assert(PpLds<256, 128, false, false>::total == 147456 && PpLds<256, 160, false, false>::total == 159744 && PpLds<256, 256, false, false>::total == 147456, "k_igemm_pp fp16, 256 rows");
static_assert(PpLds<192, 128, false, false>::total == 122880 && PpLds<192, 160, false, false>::total == 135168, "k_igemm_pp fp16, 192 rows");
static_assert(PpLds<256, 128, true, false>::total == 150528 && PpLds<256, 128, true, true>::total == 153600 && PpLds<256, 160, true, false>::total == 162816, "k_igemm_pp e4m3, 256 rows");
static_assert(PpLds<192, 128, true, false>::total == 125952 && PpLds<192, 128, true, true>::total == 129024 && PpLds<192, 160, true, false>::total == 138240 && PpLds<192, 160, true, true>::total == 141312, "k_igemm_pp e4m3, 192 rows");
static_assert(PpLds<256, 256, false, false>::ring == 131072 && PpEpiLds<256, 256>::epilogue == 147456 && PpEpiLds<256, 256>::lbt == 144384, "the one instance whose epilogue outgrows its ring");
static_assert(Pp3Lds<160, 96, false, false>::total == 163840 && Pp3Lds<128, 48, false, false>::total == 153600 && Pp3Lds<128, 24, false, false>::total == 145408, "k_igemm_pp3 fp16");
static_assert(Pp3Lds<128, 96, true, true>::total == 158720 && Pp3Lds<128, 48, true, true>::total == 134144 && Pp3Lds<128, 48, true, false>::total == 131584 && Pp3Lds<128, 24, true, false>::total == 123392, "k_igemm_pp3 e4m3");

// ---- staging -------------------------------------------------------------------------------------------------------------------------------------
// Wave `wid` owns the weight pieces (8 rows x 128 B) wid + 8 i of a BN-row tile, i < WPW = ceil(BN / 64); lane -> row 8 g + sub, source chunk `cs`
// (the XOR swizzle is applied on the SOURCE side).  gw[i] = byte offset of this lane's 16 bytes of K tile 0, TF_OOB beyond N.  ES = bytes per element.
template <int BN, int ES>
__device__ __forceinline__ void pp_weight_rows(const GemmP& p, int n0, int wid, int sub, int cs, unsigned (&gw)[(BN / 8 + 7) / 8]) {
#pragma unroll
  for (int i = 0; i < (BN / 8 + 7) / 8; ++i) {
    const int g = wid + 8 * i, n = n0 + 8 * g + sub;
    gw[i] = (g < BN / 8 && n < p.N) ? (unsigned)(n * p.K) * ES + cs * 16u : TF_OOB;
  }
}
// this wave's pieces of the weight tile at byte offset kb of every row -> LDS at `base` (the slot's weight image + wid KiB); `inside` = this lane's 16
// bytes lie inside the row (e4m3: K need not be a multiple of 128).  Returns the number of loads issued (wave-uniform).
template <int BN>
__device__ __forceinline__ int pp_stage_weights(const i4v rs_w, const unsigned (&gw)[(BN / 8 + 7) / 8], int wid, unsigned base, unsigned kb, bool inside = true) {
  constexpr int NWG = BN / 8, WPW = (NWG + 7) / 8, WREM = NWG % 8;       // the last piece only on waves < WREM where that is not 0
  int n = 0;
#pragma unroll
  for (int i = 0; i < WPW; ++i)
    if (WREM == 0 || i < WPW - 1 || wid < WREM) { dma16_w(rs_w, (gw[i] != TF_OOB && inside) ? gw[i] + kb : TF_OOB, base + (unsigned)i * 8192u); ++n; }
  return n;
}
// SGPR buffer descriptor of an activation source from the halves of its address (low word, bits 32-47) or from the pointer.  The values are wave-uniform
// by construction; the readfirstlanes are no-ops that keep them in SGPRs whatever the compiler's divergence analysis makes of the bookkeeping.
__device__ __forceinline__ i4v pp_src_rsrc(int lo, int hi, int bytes) {
  i4v rs;
  rs[0] = __builtin_amdgcn_readfirstlane(lo); rs[1] = __builtin_amdgcn_readfirstlane(hi);
  rs[2] = __builtin_amdgcn_readfirstlane(bytes); rs[3] = 0x00020000;
  return rs;
}
__device__ __forceinline__ i4v pp_src_rsrc(unsigned long long ptr, int bytes) { return pp_src_rsrc((int)(unsigned)ptr, (int)((unsigned)(ptr >> 32) & 0xffffu), bytes); }
// ... and of its codes AND scale bytes: a block-scaled e4m3 tensor holds one E8M0 byte per 32 codes behind its `bytes` codes
__device__ __forceinline__ i4v pp_scale_rsrc(int lo, int hi, int bytes) {
  const int s_nb = __builtin_amdgcn_readfirstlane(bytes);
  i4v rs;
  rs[0] = __builtin_amdgcn_readfirstlane(lo); rs[1] = __builtin_amdgcn_readfirstlane(hi);
  rs[2] = s_nb + (s_nb >> 5); rs[3] = 0x00020000;
  return rs;
}
__device__ __forceinline__ i4v pp_scale_rsrc(unsigned long long ptr, int bytes) { return pp_scale_rsrc((int)(unsigned)ptr, (int)((unsigned)(ptr >> 32) & 0xffffu), bytes); }
// Lean addressing (stride 1, no up-sampling): output row m -> pixel index of the output position and the tap-validity mask.  The input pixel of tap
// (r, s) is the position + (r - pad) W + (s - pad); bit r S + s of the mask tells whether it lies inside the image, bit 31 marks a live row (the extra
// 1x1 segment and 1x1 convolutions read the position itself).
__device__ __forceinline__ void pp_fast_pixel(int m, const GemmP& p, int& pix, int& mask) {
  int img = fast_div(m, p.dv_howo_mul, p.dv_howo_shr), rem = m - img * p.HoWo;
  int ho = fast_div(rem, p.dv_wo_mul, p.dv_wo_shr), wo = rem - ho * p.Wo;
  pix = img * p.H * p.W + ho * p.W + wo;
  unsigned bits = 0x80000000u;
  for (int r = 0; r < p.S; ++r)
    for (int s_ = 0; s_ < p.S; ++s_)
      if ((unsigned)(ho - p.pad + r) < (unsigned)p.H && (unsigned)(wo - p.pad + s_) < (unsigned)p.W) bits |= 1u << (r * p.S + s_);
  mask = (int)bits;
}

// ---- one phase's MFMAs -----------------------------------------------------------------------------------------------------------------------------
// The MFMAs of the KF k-steps held in registers, at raised priority between two scheduling barriers.  F8: one v_mfma_scale_f32_16x16x128_f8f6f4 per
// (i, j) takes both 64-byte halves of a row (KF = 2) -- e4m3 x e4m3, weights at 2^0 (their per-channel scale multiplies the accumulators later), activations
// with their block scales (block b's from lane group b, byte 0 of sx[j]).
// PIN (F8): pin the results behind the block.  The intrinsic has no side effect, and without a use in its phase the compiler sinks a whole slab's MFMAs of
// k_igemm_pp3 behind the last barrier of the slab and parks the fragments in scratch; k_igemm_pp's tile loop does not need it.
template <bool F8, bool BF, int KF, int NI, int MJ, bool PIN = false>
__device__ __forceinline__ void pp_mma(const h8 (&wf)[KF][NI], const h8 (&xf)[KF][MJ], f4 (&acc)[NI][MJ], const int (&sx)[MJ]) {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
  if constexpr (F8) {
    typedef int v8i __attribute__((ext_vector_type(8)));
    typedef int v4i __attribute__((ext_vector_type(4)));
    v8i xv[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      v4i lo = __builtin_bit_cast(v4i, xf[0][j]), hi = __builtin_bit_cast(v4i, xf[KF - 1][j]);
      xv[j] = (v8i){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      v4i lo = __builtin_bit_cast(v4i, wf[0][i]), hi = __builtin_bit_cast(v4i, wf[KF - 1][i]);
      const v8i wv = (v8i){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
      for (int j = 0; j < MJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv, xv[j], acc[i][j], 0, 0, 0, 0x7F7F7F7F, 0, sx[j]);
    }
    if constexpr (PIN) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MJ; ++j) asm volatile("" :: "v"(acc[i][j]));
    }
  } else {
#pragma unroll
    for (int f = 0; f < KF; ++f)
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MJ; ++j) acc[i][j] = mfma16<BF>(wf[f][i], xf[f][j], acc[i][j]);
  }
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void pp_barrier() {
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- behind the K loop -----------------------------------------------------------------------------------------------------------------------------
// e4m3: the per-output-channel weight scales on the accumulators (this lane's 4 consecutive channels of every n-tile; nb = first channel of the wave tile)
template <int NI, int MJ>
__device__ __forceinline__ void pp_apply_wscale(const GemmP& p, f4 (&acc)[NI][MJ], int nb, int lg) {
  if (!p.wscale) return;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = nb + i * 16 + lg * 4;
    f4 w = {1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) if (n + e < p.N) w[e] = p.wscale[n + e];
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] *= w;
  }
}
// Bias and time-embedding values of the tile's columns, fetched in front of the K loop (latency under it) and handed to the epilogue through the LDS
// table at PpEpiLds::lbt: thread t < BN holds column n0 + t.  A tile spans at most two images (TWO; the host admits k_igemm_pp only where HoWo >= BM;
// a tile of k_igemm_pp3 lies inside one): c0 / c1 = the time embedding of image img0 / img0 + 1.  `on` = false: a split-K launch, the reducer adds them.
struct PpBias { float b, c0, c1; };
template <int BN, bool BF, bool TWO>
__device__ __forceinline__ PpBias pp_bias_prefetch(const GemmP& p, int n0, int tid, int img0, bool on) {
  PpBias lb = {0.f, 0.f, 0.f};
  if (tid < BN && n0 + tid < p.N && on) {
    if (p.bias) lb.b = e2f<BF>(p.bias[n0 + tid]);
    if (p.bias_nc) {
      lb.c0 = e2f<BF>(p.bias_nc[(long long)img0 * p.bias_nc_stride + n0 + tid]);
      if constexpr (TWO) { if ((img0 + 1) * p.HoWo < p.M) lb.c1 = e2f<BF>(p.bias_nc[(long long)(img0 + 1) * p.bias_nc_stride + n0 + tid]); }
    }
  }
  return lb;
}
// The epilogue: the accumulators go through the 2 x 2-wave-tile scratch of k_igemm in two passes of BM / 2 rows (wave (wm, wn) is quadrant (wm & 1, wn)
// of pass wm >> 1), so bias / time embedding / residual / GEGLU / split-K partials / GroupNorm statistics are the shared code, chunked as a BM / 2-row
// tile.  `pre` runs in a wave of the pass in front of its igemm_scratch_write (k_igemm_pp<LNF>: the rows' LayerNorm statistics into the table at
// PpEpiLds::ln_stats).  OUT8 = 2: a launch with p.out8 stores block-scaled e4m3 (GEGLU; igemm_epilogue's OUT8), fp16 bias / residual.
template <int BM, int BN, bool BF, int OUT8, int NI, int MJ, class Pre>
__device__ __forceinline__ void pp_epilogue(const GemmP& p, char* smem, f4 (&acc)[NI][MJ], const f4 (&csum)[NI], const PpBias& lb, int m0, int n0, int split, int img0, int tid, Pre&& pre) {
  using L = PpEpiLds<BM, BN>;
  constexpr int BS = L::BS;
  const int lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wid & 3, wn = wid >> 2;
  float* const lbt = reinterpret_cast<float*>(smem + L::lbt);
  if (tid < BN) { lbt[tid] = lb.b; lbt[BN + tid] = lb.c0; lbt[2 * BN + tid] = lb.c1; }                       // (visible behind the first pass's barrier)
  const int lb_m1 = (img0 + 1) * p.HoWo;
#pragma unroll
  for (int sm = 0; sm < 2; ++sm) {
    if ((wm >> 1) == sm) {
      pre();
      igemm_scratch_write<BS, BN>(p, acc, csum, smem, (wm & 1) | (wn << 1), lane);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pp_barrier();
    // (two items' loads in flight at a time: half of the accumulators is still live during the first pass)
    if (OUT8 && p.out8) igemm_epilogue<BS, BN, OUT8, false, 2, true>(p, smem, m0 + sm * BS, n0, split, wm, wn, lane, lbt, n0, lb_m1);
    else igemm_epilogue<BS, BN, 0, BF, 2, true>(p, smem, m0 + sm * BS, n0, split, wm, wn, lane, lbt, n0, lb_m1);
    if (p.gn_part && m0 + sm * BS < p.M) igemm_gn_stats<BS, BN>(p, smem, m0 + sm * BS, n0, wm, wn, lane);   // (block-uniform: the barrier inside is safe)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    pp_barrier();
  }
}
