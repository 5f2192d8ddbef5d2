// Part of the implicit-GEMM family of csrc/gemm.hip (see its head comment).
// What the three persistent short-K kernels have in common -- k_gemm_c4 (gemm_c4.h), k_gemm_c8 (gemm_c8.h), k_gemm_ar (gemm_ar.h) -- each piece ONCE:
//   the chunked walk (the tile-order decode is tile_decode of gemm_common.h); a wave's staging rows and the LDS-DMA of one K tile (SkStager); the fragment address, the read of a
//   32-deep half, its MFMAs and LayerNorm row sums; the bias / column-sum request at the head of a tile; the LayerNorm fold + bias on the accumulators;
//   the row-sum reduce (and the partner exchange of c4 / c8); the rounding of a 16-row quarter; the transposing store of a wave tile (c4 / c8); and
//   the launchers' CU count, LDS attribute and chunk rule.
// What is NOT here is what differs: the ring protocol of each kernel (slots, barriers, the counted vmcnt waits) and its place in LDS.
// Every wave tile is 64 x 64 (MJ = NI = 4 MFMA tiles of 16 x 16): a lane ends up with 4 consecutive (packed) channels of a pixel per (i, j).
// The counted waits of the kernels rest on the instruction counts of these pieces: SkStager issues exactly NA + NWP LDS-DMA pieces per wave and K tile,
// sk_request NI loads per operand it is given, sk_store_wave_tile sk_wave_tile_stores() stores on an interior tile without a residual.
#pragma once
#include "gemm_common.h"
#include <stdlib.h>
#include <initializer_list>

// ---- tile order and walk -------------------------------------------------------------------------------------------------------------------------
// a block's tiles: chunks of `chunk` consecutive tiles of the list, the chunks strided by the grid.  Consecutive tiles (n-fastest order) share their
// rows -- L1 / L2 lines, and with the LayerNorm fold the row statistics, computed for the first tile of a run only -- while the blocks running at the
// same time stay next to each other in the list (whole runs per block, each block on rows of its own, cost the wide-N shapes 5-15 %).
// (q, e) = chunk index, tile inside the chunk; -> the next tile index or -1
__device__ __forceinline__ int sk_next_tile(int& q, int& e, int chunk, int gstep, int ntiles) {
  if (e + 1 < chunk && q * chunk + e + 1 < ntiles) { ++e; return q * chunk + e; }
  q += gstep; e = 0;
  return q * chunk < ntiles ? q * chunk : -1;
}

// ---- staging -------------------------------------------------------------------------------------------------------------------------------------
// One of NW staging waves (w = its index): of a 128-byte-row operand tile it takes the 8-row pieces w + NW i -- rows 8 (w + NW i) + sub of the tile,
// NA pieces of the activation tile and NWP of the weight tile per K tile -- one 16-byte chunk per lane, the LDS image lane-linear (1 KiB per piece, the
// pieces of a wave NW KiB apart) with the XOR swizzle applied to the SOURCE chunk.  Rows beyond M / N read TF_OOB: zeros in LDS.
template <int NW, int NA, int NWP>
struct SkStager {
  i4v rs_x1, rs_x2, rs_w;
  int C1, C2, M, N, K;
  int w, sub, cs;
  int am[NA];
  unsigned gw[NWP];
  __device__ __forceinline__ SkStager(const GemmP& p, int w_, int lane)
      : rs_x1(raw_rsrc(p.x, p.x_bytes)), rs_x2(raw_rsrc(p.x2 ? p.x2 : p.x, p.x2_bytes)), rs_w(raw_rsrc(p.w, p.w_bytes)), C1(p.C1), C2(p.C2), M(p.M), N(p.N), K(p.K), w(w_), sub(lane >> 3) {
    cs = (lane & 7) ^ ((4 * (w & 1) + (sub >> 1)) & 7);   // source chunk: pieces of a wave are NW (4 or 8) apart, so 8 g's parity is the wave's
  }
  __device__ __forceinline__ void rows_a(int m0) {
#pragma unroll
    for (int i = 0; i < NA; ++i) { const int m = m0 + 8 * (w + NW * i) + sub; am[i] = m < M ? m : -1; }
  }
  __device__ __forceinline__ void rows_w(int n0) {
#pragma unroll
    for (int i = 0; i < NWP; ++i) { const int n = n0 + 8 * (w + NW * i) + sub; gw[i] = n < N ? (unsigned)(n * K + cs * 8) * 2u : TF_OOB; }
  }
  // K tile kt of the rows in am[] -> the activation image at LDS offset `base`; the concat pair is two sources with a row pitch each (the seam lies on the 64 grid)
  __device__ __forceinline__ void stage_a(int kt, unsigned base) const {
    const int c = kt * 64;
    const bool second = c >= C1;
    const int ld = second ? C2 : C1;
    const int cc = (second ? c - C1 : c) + cs * 8;
    const i4v rs = second ? rs_x2 : rs_x1;
#pragma unroll
    for (int i = 0; i < NA; ++i) dma16(rs, am[i] >= 0 ? (unsigned)(am[i] * ld + cc) * 2u : TF_OOB, base + (unsigned)w * 1024u + (unsigned)i * (NW * 1024u));
  }
  // K tile kt of the rows in gw[] -> the weight image at LDS offset `base`
  __device__ __forceinline__ void stage_w(int kt, unsigned base) const {
#pragma unroll
    for (int i = 0; i < NWP; ++i) dma16_w(rs_w, gw[i] != TF_OOB ? gw[i] + (unsigned)kt * 128u : TF_OOB, base + (unsigned)w * 1024u + (unsigned)i * (NW * 1024u));
  }
};

// ---- one K step of a 64 x 64 wave tile -------------------------------------------------------------------------------------------------------------
// this lane's fragment inside a 16-row x 128-byte MFMA tile of an operand image: row lr, 16-byte chunk lg (the first 32-deep half) swizzled as staged
__device__ __forceinline__ int sk_frag_off(int lane) {
  const int lr = lane & 15, lg = lane >> 4;
  return lr * 128 + ((lg ^ ((lr >> 1) & 7)) << 4);
}
// the four fragments of 32-deep half f of a K tile: `off` = image offset of the wave tile's first MFMA tile + sk_frag_off
__device__ __forceinline__ void sk_read_half(h8 (&fr)[4], const char* base, int off, int f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) fr[i] = *reinterpret_cast<const h8*>(base + ((off + i * 2048) ^ (f * 64)));
}
template <bool BF>
__device__ __forceinline__ void sk_mma_half(const h8 (&wf)[4], const h8 (&xf)[4], f4 (&acc)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mfma16<BF>(wf[i], xf[j], acc[i][j]);
}
// LayerNorm row statistics from the fragments the wave multiplies: this lane's partial (sum, sum of squares) of row j * 16 + lr over one half
template <bool BF>
__device__ __forceinline__ void sk_stats_half(const h8 (&xf)[4], float (&ls)[4], float (&lq)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) dot2_stats<BF>(xf[j], ls[j], lq[j]);
}

// ---- head of a tile ------------------------------------------------------------------------------------------------------------------------------
// bias (and LayerNorm column sums) of this lane's columns, nb = first (packed) column of the wave tile: requested at the head of a tile, consumed behind
// the K loop -- and BEFORE the next tile's prefetch is issued: the compiler counts only its own loads, so a wait for them placed behind the asm LDS-DMA
// would wait for the DMA too.  The values stay as loaded (a conversion here would put the compiler's vmcnt(0) here); sk_request_pin, behind the K
// loop, is where they are used from: nothing of the fold moves in front of the K loop.  Issues 4 loads per operand present.
template <bool LNF>
__device__ __forceinline__ void sk_request(const GemmP& p, int nb, int lg, h4 (&braw)[4], f4 (&cq)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    braw[i] = (h4){(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f}; cq[i] = (f4){0.f, 0.f, 0.f, 0.f};
    int n = nb + i * 16 + lg * 4;
    n = n + 3 < p.N ? n : 0;                               // columns beyond N are never stored: any readable address will do (no masked load)
    if (p.bias) braw[i] = *reinterpret_cast<const h4*>(p.bias + n);
    if constexpr (LNF) cq[i] = *reinterpret_cast<const f4*>(p.ln_colsum + n);
  }
}
template <bool LNF>
__device__ __forceinline__ void sk_request_pin(h4 (&braw)[4], f4 (&cq)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    asm volatile("" : "+v"(braw[i]));
    if constexpr (LNF) asm volatile("" : "+v"(cq[i]));
  }
}

// ---- LayerNorm fold --------------------------------------------------------------------------------------------------------------------------------
// a row's sums over the four lanes (lg) that hold it
__device__ __forceinline__ void sk_row_reduce(float& s, float& q) {
  s += __shfl_xor(s, 16, 64); q += __shfl_xor(q, 16, 64);
  s += __shfl_xor(s, 32, 64); q += __shfl_xor(q, 32, 64);
}
__device__ __forceinline__ void sk_mean_rstd(float s, float q, float invK, float eps, float& mean, float& rstd) {
  mean = s * invK;
  rstd = rsqrtf(fmaxf(q * invK - mean * mean, 0.f) + eps);
}
// k_gemm_c4 / k_gemm_c8, where the two waves that share 64 rows take one 32-deep half of every K tile each: this wave's half of the row sums -> LDS
// (stats: [wave][64 rows]) in front of the barrier that ends the K loop ...
__device__ __forceinline__ void sk_rowsum_put(f2* stats, int wid, int lane, float (&ls)[4], float (&lq)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sk_row_reduce(ls[j], lq[j]);
    if ((lane >> 4) == 0) stats[wid * 64 + j * 16 + (lane & 15)] = (f2){ls[j], lq[j]};
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (a raw s_barrier does not wait for LDS stores)
}
// ... and the partner's half (wave `partner`: same rows, the other half) back behind it
__device__ __forceinline__ void sk_rowsum_get(const f2* stats, int partner, int lane, const float (&ls)[4], const float (&lq)[4], int K, float eps, float (&mean)[4], float (&rstd)[4]) {
  const float invK = 1.0f / (float)K;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f2 o_ = stats[partner * 64 + j * 16 + (lane & 15)];
    sk_mean_rstd(ls[j] + o_[0], lq[j] + o_[1], invK, eps, mean[j], rstd[j]);
  }
}
// y = rstd[m] (x . w'^T - mean[m] colsum[n]) + bias'[n] on the accumulators (registers)
template <bool LNF, bool BF>
__device__ __forceinline__ void sk_fold(f4 (&acc)[4][4], const float (&mean)[4], const float (&rstd)[4], const f4 (&cq)[4], const h4 (&braw)[4]) {
  if constexpr (LNF) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = rstd[j] * (acc[i][j] - mean[j] * cq[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] += (f4){e2f<BF>(braw[i][0]), e2f<BF>(braw[i][1]), e2f<BF>(braw[i][2]), e2f<BF>(braw[i][3])};
}

// ---- output --------------------------------------------------------------------------------------------------------------------------------------
// quarter j (16 rows) of the wave tile rounded to 16 bits: o[i] = this lane's 4 channels of column tile i, or with GEGLU (value / gate column tiles
// alternate: ff/nn.py:10-12) of output column tile i = value 2 i x gelu(gate 2 i + 1)
template <bool GG, bool BF>
__device__ __forceinline__ void sk_round_quarter(const f4 (&acc)[4][4], int j, h4 (&o)[GG ? 2 : 4]) {
  if constexpr (GG) {
#pragma unroll
    for (int i = 0; i < 4; i += 2)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[i >> 1][e] = f2e<BF>(acc[i][j][e] * gelu_f(acc[i + 1][j][e]));
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[i][e] = f2e<BF>(acc[i][j][e]);
  }
}
// The epilogue of k_gemm_c4 / k_gemm_c8, without a block barrier: the folded accumulators of a wave tile (rows from m0w, packed columns from nbc) rounded,
// transposed through the PRIVATE per-wave patch at LDS offset pa (32 rows x (128 + 16) bytes) half a wave tile at a time (pixel tiles j = 2 h, 2 h + 1)
// into 16-byte row segments of 64 (32 with GEGLU) outputs, residual added there, stored.  Nothing waits for the stores.
// An interior tile without a residual stores 2 halves x 32 rows x cpr chunks / 64 lanes = 8 (GEGLU: 4) times per wave, every lane active:
__device__ __forceinline__ int sk_wave_tile_stores(bool geglu) { return geglu ? 4 : 8; }
template <bool LNF, bool BF>
__device__ __forceinline__ void sk_store_wave_tile(const GemmP& p, const f4 (&acc)[4][4], unsigned pa, int m0w, int nbc, int lane) {
  const int lr = lane & 15, lg = lane >> 4;
  const int M_ = p.M;
  const bool geglu = p.act == 1;
  const int No = geglu ? p.N >> 1 : p.N;
  const int ocol0 = geglu ? (nbc >> 1) : nbc;              // packed column -> output column (n >> 5) * 16 + (n & 15) = n / 2 for n a multiple of 32
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int j = 2 * h + jj;
      const unsigned rowa = pa + (unsigned)(jj * 16 + lr) * 144u;
      if (geglu) {
        h4 o[2];
        sk_round_quarter<true, BF>(acc, j, o);
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("ds_write_b64 %0, %1" ::"v"(rowa + (unsigned)(i * 32 + lg * 8)), "v"(o[i]) : "memory");
      } else {
        h4 o[4];
        sk_round_quarter<false, BF>(acc, j, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("ds_write_b64 %0, %1" ::"v"(rowa + (unsigned)(i * 32 + lg * 8)), "v"(o[i]) : "memory");
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // read back as rows: 32 rows x 8 or 4 16-byte chunks (a shift, not a divide: the runtime quotient cost ~40 VALU instructions per use)
    const int csh = geglu ? 2 : 3, cpr = 1 << csh;
    // the residual rows of this half are requested up front -- as one loop the residual load of every iteration sat behind the previous
    // iteration's store and in front of its own use: four serial global round trips per half
    h8 rres[4];
    if (!LNF && p.residual) {                              // (no LayerNorm-folded launch of the step carries a residual: that instance keeps its registers)
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int idx = lane + 64 * it;
        const int row = idx >> csh, c8 = idx & (cpr - 1);
        const int m = m0w + h * 32 + row, no = ocol0 + c8 * 8;
        // (a segment that is not stored reads any readable address: four loads in a row whatever the edge.  Loaded under `if`, the moved code compiled to two loads, a
        // vmcnt(0) for a register copy, and the other two: two round trips per half)
        const long long o = (idx < 32 * cpr && m < M_ && no < No) ? (long long)m * No + no : 0;
        rres[it] = *reinterpret_cast<const h8*>(p.residual + o);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = lane + 64 * it;
      if (idx >= 32 * cpr) break;                          // (GEGLU: two iterations)
      const int row = idx >> csh, c8 = idx & (cpr - 1);
      const int m = m0w + h * 32 + row, no = ocol0 + c8 * 8;
      h8 v;
      asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(pa + (unsigned)row * 144u + (unsigned)c8 * 16u) : "memory");
      if (m < M_ && no < No) {
        const long long o = (long long)m * No + no;
        if (p.residual) { const h8 r = LNF ? *reinterpret_cast<const h8*>(p.residual + o) : rres[it]; for (int e = 0; e < 8; ++e) v[e] = f2e<BF>(e2f<BF>(v[e]) + e2f<BF>(r[e])); }
        *reinterpret_cast<h8*>(p.y + o) = v;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ---- launchers (host) ------------------------------------------------------------------------------------------------------------------------------
static int shortk_num_cus() {
  static int n = 0;
  if (!n) { int dev = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256; }
  return n;
}
// the dynamic LDS of every instance of a launcher, once (`done` is the launcher's)
static int shortk_set_lds(bool& done, int smem, std::initializer_list<const void*> kernels) {
  if (done) return TF_OK;
  for (const void* k : kernels) TF_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
  done = true;
  return TF_OK;
}
// consecutive tiles per block of the chunked walk.  Without the LayerNorm fold: one (chunks of 2-8 were 2-8 % faster on three narrow-N shapes and up to
// 6x slower wherever they left fewer chunks than blocks).  With it (n-fastest order): 4 or 2 while that still leaves per_cu chunks per CU (4 x the resident
// blocks: every block still gets >= 4 chunks) -- the statistics of a row block are computed once per chunk
static int shortk_chunk(const GemmP& p, int tiles, int per_cu) {
  if (!p.ln_colsum || p.order != 0) return 1;
  const int floor_ = per_cu * shortk_num_cus();
  return tiles / 4 >= floor_ ? 4 : tiles / 2 >= floor_ ? 2 : 1;
}
