// The split-K reduce kernels of the GEMM family -- partial slabs summed in split order + the epilogue, optionally with the GroupNorm statistics of the
// output, optionally with the GroupNorm itself applied in the same launch -- and the one host function that launches them (gemm_reduce.h).
#include "gemm_reduce.h"

// Split-K partial slabs are fp32 or -- round 4, GemmP::part16 -- fp16 (half the bytes of the seam: a slab is written once and read once, both
// through HBM / L2; the reducer accumulates in fp32 in split order either way).  PT = the slab's element type.
template <typename PT> __device__ __forceinline__ f4 part_load4(const PT* p);
template <> __device__ __forceinline__ f4 part_load4<float>(const float* p) { return *reinterpret_cast<const f4*>(p); }
template <> __device__ __forceinline__ f4 part_load4<half_t>(const half_t* p) {
  const h4 h = *reinterpret_cast<const h4*>(p);
  return (f4){(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
// The split partials of one element quad, summed in split order with NB independent loads in flight.  The loads are UNCONDITIONAL -- a slab index
// past the last one re-reads the last slab and its value is dropped -- because a load under `z < splitk` compiles to load / wait / branch one slab at a
// time (round 4: the reducers spent 8-16 serial L2 latencies per element that way, 14 us for a launch that moves 5 MB).  NB is the smallest of 2 / 4 /
// 8 / 16 that covers splitk in one batch where it can: no redundant loads for the common split counts.
template <typename PT, int NB, bool VS = true>
__device__ __forceinline__ f4 sum_partials_nb(const PT* __restrict__ partial, long long total, long long e0, int splitk) {
  f4 v = {0.f, 0.f, 0.f, 0.f};
  // (the slab stride as a per-lane value: with a uniform stride the compiler keeps NB 64-bit slab bases in SGPRs -- 26-41 of them spilled in the
  // fp16-slab instances, VERDICT r4 -- where one 64-bit VALU multiply-add per load does)
  // VS = false (k_splitk_reduce_gn_apply: 128-VGPR budget at 1024 threads, where the per-lane addresses spill VECTOR registers instead): uniform stride
  int zv_ = 0;
  if constexpr (VS) asm volatile("v_mov_b32 %0, 0" : "=v"(zv_));
  const long long stride_v = total + (long long)zv_;
  for (int z0 = 0; z0 < splitk; z0 += NB) {
    f4 u[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) u[i] = part_load4<PT>(partial + (long long)min(z0 + i, splitk - 1) * stride_v + e0);
#pragma unroll
    for (int i = 0; i < NB; ++i) v += z0 + i < splitk ? u[i] : (f4){0.f, 0.f, 0.f, 0.f};
  }
  return v;
}
template <typename PT, bool VS = true>
__device__ __forceinline__ f4 sum_partials(const PT* __restrict__ partial, long long total, long long e0, int splitk) {
  if (splitk <= 2) return sum_partials_nb<PT, 2, VS>(partial, total, e0, splitk);
  if (splitk <= 4) return sum_partials_nb<PT, 4, VS>(partial, total, e0, splitk);
  if (sizeof(PT) == 2 && splitk > 8) return sum_partials_nb<PT, 16, VS>(partial, total, e0, splitk);
  return sum_partials_nb<PT, 8, VS>(partial, total, e0, splitk);
}
// Two neighbouring element quads of an fp16 slab with ONE 16-byte load per split (the group-major slabs of k_splitk_reduce_gn_apply: a wave
// instruction covers 1 KiB = eight whole lines), each summed in split order exactly as sum_partials_nb sums one: the same adds in the same order.
// At most 8 loads in flight: as many bytes as sum_partials' 16 of 8.
template <int NB>
__device__ __forceinline__ void sum_partials16_nb(const half_t* __restrict__ partial, long long total, long long e0, int splitk, f4& lo, f4& hi) {
  for (int z0 = 0; z0 < splitk; z0 += NB) {
    h8 u[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) u[i] = *reinterpret_cast<const h8*>(partial + (long long)min(z0 + i, splitk - 1) * total + e0);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      lo += z0 + i < splitk ? (f4){(float)u[i][0], (float)u[i][1], (float)u[i][2], (float)u[i][3]} : (f4){0.f, 0.f, 0.f, 0.f};
      hi += z0 + i < splitk ? (f4){(float)u[i][4], (float)u[i][5], (float)u[i][6], (float)u[i][7]} : (f4){0.f, 0.f, 0.f, 0.f};
    }
  }
}
__device__ __forceinline__ void sum_partials16(const half_t* __restrict__ partial, long long total, long long e0, int splitk, f4& lo, f4& hi) {
  if (splitk <= 2) return sum_partials16_nb<2>(partial, total, e0, splitk, lo, hi);
  if (splitk <= 4) return sum_partials16_nb<4>(partial, total, e0, splitk, lo, hi);
  return sum_partials16_nb<8>(partial, total, e0, splitk, lo, hi);
}
// split-K reduce + epilogue: y[m,n] = sum_z partial[z,m,n] + bias + bias_nc + residual   (N % 4 == 0 fast path)
// BF: bias / bias_nc / residual / gamma / beta / y / z hold bfloat16 (containers as in gemm_common.h: e2f / f2e)
template <typename PT, bool BF = false>
__global__ void __launch_bounds__(256) k_splitk_reduce(half_t* __restrict__ y, const PT* __restrict__ partial, const half_t* __restrict__ bias,
                                                       const half_t* __restrict__ bias_nc, const half_t* __restrict__ residual, int M, int N,
                                                       int HoWo, int splitk, long long bnc_stride) {
  long long total = (long long)M * N;
  long long gs = (long long)gridDim.x * 256;
  if ((N & 3) == 0) {
    long long nv = total >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += gs) {
      long long e0 = i << 2;
      int m = (int)(e0 / N), n = (int)(e0 - (long long)m * N);
      f4 v = sum_partials<PT>(partial, total, e0, splitk);
      if (bias) { h4 b = *reinterpret_cast<const h4*>(bias + n); for (int e = 0; e < 4; ++e) v[e] += e2f<BF>(b[e]); }
      if (bias_nc) { h4 b = *reinterpret_cast<const h4*>(bias_nc + (long long)(m / HoWo) * bnc_stride + n); for (int e = 0; e < 4; ++e) v[e] += e2f<BF>(b[e]); }
      if (residual) { h4 b = *reinterpret_cast<const h4*>(residual + e0); for (int e = 0; e < 4; ++e) v[e] += e2f<BF>(b[e]); }
      h4 o;
      for (int e = 0; e < 4; ++e) o[e] = f2e<BF>(v[e]);
      *reinterpret_cast<h4*>(y + e0) = o;
    }
  } else {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += gs) {
      int m = (int)(i / N), n = (int)(i - (long long)m * N);
      float v = 0.f;
      for (int z = 0; z < splitk; ++z) v += (float)partial[(long long)z * total + i];
      if (bias) v += e2f<BF>(bias[n]);
      if (bias_nc) v += e2f<BF>(bias_nc[(long long)(m / HoWo) * bnc_stride + n]);
      if (residual) v += e2f<BF>(residual[i]);
      y[i] = f2e<BF>(v);
    }
  }
}

// split-K reduce + epilogue + GroupNorm statistics of the output (tf_conv2d_fused_f16 on a split-K shape): a block owns R
// whole output rows (R = HoWo / chunks); thread t owns column quad t % nq and the rows r = t / nq (mod RL), so the
// per-channel sums stay in its registers; row lanes and channels -> groups meet through LDS in a fixed order.
// The split partials of an element are fetched 8 at a time (independent loads) and added in split order.
template <typename PT, bool BF = false>
__global__ void __launch_bounds__(1024) k_splitk_reduce_gn(half_t* __restrict__ y, const PT* __restrict__ partial, const half_t* __restrict__ bias,
                                                           const half_t* __restrict__ bias_nc, const half_t* __restrict__ residual, int M, int N,
                                                           int HoWo, int splitk, long long bnc_stride, float* __restrict__ gn_part, int G, int cpg,
                                                           int chunks, int R, int RL) {
  extern __shared__ float chan[];                        // [RL][N][2]
  const long long total = (long long)M * N;
  const int m_first = blockIdx.x * R;
  const int nq = N >> 2;
  const int rl = threadIdx.x / nq, q0 = threadIdx.x - rl * nq;
  if (rl < RL) {
    const int n = q0 << 2;
    f4 cs = {0.f, 0.f, 0.f, 0.f}, cq = {0.f, 0.f, 0.f, 0.f};
    f4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) { h4 b = *reinterpret_cast<const h4*>(bias + n); for (int e = 0; e < 4; ++e) bv[e] = e2f<BF>(b[e]); }
    for (int r = rl; r < R; r += RL) {
      const int m = m_first + r;
      const long long e0 = (long long)m * N + n;
      h4 bnc = {0, 0, 0, 0}, res = {0, 0, 0, 0};
      if (bias_nc) bnc = *reinterpret_cast<const h4*>(bias_nc + (long long)(m / HoWo) * bnc_stride + n);
      if (residual) res = *reinterpret_cast<const h4*>(residual + e0);
      f4 v = sum_partials<PT>(partial, total, e0, splitk);
      v += bv;
      for (int e = 0; e < 4; ++e) v[e] += e2f<BF>(bnc[e]);
      for (int e = 0; e < 4; ++e) v[e] += e2f<BF>(res[e]);
      h4 o;
      for (int e = 0; e < 4; ++e) { o[e] = f2e<BF>(v[e]); float f = e2f<BF>(o[e]); cs[e] += f; cq[e] += f * f; }
      *reinterpret_cast<h4*>(y + e0) = o;
    }
    float* ch = chan + (long long)rl * N * 2;
    for (int e = 0; e < 4; ++e) { ch[2 * (n + e)] = cs[e]; ch[2 * (n + e) + 1] = cq[e]; }
  }
  __syncthreads();
  // one wave per group (round-robin): lane = channel of the group (cpg <= 64), RL row-lane reads, shuffle tree
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int img = m_first / HoWo, slot = (m_first - img * HoWo) / R;
  for (int g = wv; g < G; g += nw) {
    float S = 0.f, Q = 0.f;
    if (lane < cpg) {
      const int c = g * cpg + lane;
      for (int l = 0; l < RL; ++l) { S += chan[((long long)l * N + c) * 2]; Q += chan[((long long)l * N + c) * 2 + 1]; }
    }
    S = wave_sum(S); Q = wave_sum(Q);
    if (lane == 0) {
      float* dst = gn_part + ((long long)(img * chunks + slot) * G + g) * 2;
      dst[0] = S; dst[1] = Q;
    }
  }
}

// split-K reduce + epilogue + GroupNorm of the output, statistics AND apply, in one launch (conv -> GroupNorm -> SiLU of
// vision/resnet.py:17-22 behind a split-K conv): a block owns ALL rows of one image for `gpb` whole groups (CW = gpb * cpg channels),
// so the statistics are complete inside the block and no second launch has to wait for them.  Thread t holds the column quad
// t % CV of rows t / CV + k * RPS (k < RGA_MAXR) in registers: partials summed in split order (8 loads in flight), + bias + bias_nc +
// residual, rounded to fp16 (y, optional), per-channel sums in registers -> LDS -> fixed-order fold -> (mean, rstd) -> z = silu?(y a + b).
// Also leaves the (sum, sum of squares) of every group as a one-chunk partial table, so y.gn stays available to later consumers.
// GM (GemmP::slab_gm, gpb == 1): the slabs are group-major -- the block's partials are ONE run of HoWo cpg elements per split, and quad v of row
// rl + k RPS is quad t + k RPS CV of that run: consecutive lanes, consecutive quads.  GM == 1 loads a quad per lane (fp32 slabs: 16 bytes).  GM == 2
// (fp16 slabs; RPS CV and HoWo CV even): sweeps go in pairs (k, k + 1) -- the even lane of a lane pair loads 16 bytes = both lanes' quads of sweep k,
// the odd lane both lanes' quads of sweep k + 1, each sums its two quads over the splits and the pair swaps one fp32 sum each way, so every lane
// ends up with the very sums, added in the very order, it computes on its own under GM == 0 / 1: y, z and the table do not depend on GM.
#define RGA_MAXR 8
template <typename PT, bool BF = false, int GM = 0>
__global__ void __launch_bounds__(1024) k_splitk_reduce_gn_apply(half_t* __restrict__ y, half_t* __restrict__ z, const PT* __restrict__ partial,
                                                                 const half_t* __restrict__ bias, const half_t* __restrict__ bias_nc,
                                                                 const half_t* __restrict__ residual, int M, int N, int HoWo, int splitk, long long bnc_stride,
                                                                 float* __restrict__ gn_part, int G, int cpg, int gpb, const half_t* __restrict__ gamma,
                                                                 const half_t* __restrict__ beta, float eps, int do_silu, int RPS, int CV) {
  extern __shared__ float sm[];                          // [RPS][CW][2], then [parts][CW][2] behind it, then [gpb][2]
  const int nb = G / gpb;
  const int img = blockIdx.x / nb, gs = blockIdx.x - img * nb;
  const int CW = gpb * cpg, c0 = gs * CW;
  const int t = threadIdx.x;
  const int rl = t / CV, v = t - rl * CV;
  const bool act = rl < RPS;
  const int n = c0 + v * 4;
  const long long total = (long long)M * N;
  f4 bv = {0.f, 0.f, 0.f, 0.f};
  h4 bnc = {0, 0, 0, 0};
  h4 gm = {f2e<BF>(1.f), f2e<BF>(1.f), f2e<BF>(1.f), f2e<BF>(1.f)}, bt = {0, 0, 0, 0};               // (fetched here, under the partials' latency: behind the block barriers they would be one more serial L2 round trip)
  if (act) {
    if (bias) { h4 b = *reinterpret_cast<const h4*>(bias + n); for (int e = 0; e < 4; ++e) bv[e] = e2f<BF>(b[e]); }
    if (bias_nc) bnc = *reinterpret_cast<const h4*>(bias_nc + (long long)img * bnc_stride + n);
    if (gamma) { gm = *reinterpret_cast<const h4*>(gamma + n); bt = *reinterpret_cast<const h4*>(beta + n); }
  }
  h4 out[RGA_MAXR];
  f4 cs = {0.f, 0.f, 0.f, 0.f}, cq = {0.f, 0.f, 0.f, 0.f};
  const PT* const slab = partial + (long long)blockIdx.x * HoWo * cpg;   // GM: the block's run inside split 0's slab
  const int S = RPS * CV;                                                  // GM: quads per sweep
  f4 acc_next = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < RGA_MAXR; ++k) {
    const int r = rl + k * RPS;
    out[k] = (h4){0, 0, 0, 0};
    f4 acc_pair = acc_next;
    if constexpr (GM == 2) {
      if ((k & 1) == 0) {                                    // (outside every divergent branch: all 64 lanes take part in the swap)
        const int odd = t & 1, q = (t - odd) + (k + odd) * S;
        f4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (act && q < HoWo * CV) sum_partials16(reinterpret_cast<const half_t*>(slab), total, 4LL * q, splitk, lo, hi);
        const f4 send = odd ? lo : hi;
        f4 recv;
        for (int e = 0; e < 4; ++e) recv[e] = __shfl_xor(send[e], 1, 64);
        acc_pair = odd ? recv : lo;
        acc_next = odd ? hi : recv;
      }
    }
    if (act && r < HoWo) {
      const long long e0 = ((long long)img * HoWo + r) * N + n;
      h4 res = {0, 0, 0, 0};
      if (residual) res = *reinterpret_cast<const h4*>(residual + e0);
      f4 acc;
      if constexpr (GM == 2) acc = acc_pair;
      else if constexpr (GM == 1) acc = sum_partials<PT, false>(slab, total, 4LL * (t + k * S), splitk);
      else acc = sum_partials<PT, false>(partial, total, e0, splitk);
      acc += bv;
      for (int e = 0; e < 4; ++e) acc[e] += e2f<BF>(bnc[e]);
      for (int e = 0; e < 4; ++e) acc[e] += e2f<BF>(res[e]);
      h4 o;
      for (int e = 0; e < 4; ++e) { o[e] = f2e<BF>(acc[e]); float f = e2f<BF>(o[e]); cs[e] += f; cq[e] += f * f; }
      out[k] = o;
      if (y) *reinterpret_cast<h4*>(y + e0) = o;
    }
  }
  f2* col = reinterpret_cast<f2*>(sm);                   // [RPS][CW]
  if (act) for (int e = 0; e < 4; ++e) col[rl * CW + v * 4 + e] = (f2){cs[e], cq[e]};
  __syncthreads();
  // fold 1: thread (part, c) sums the row lanes part, part + parts, ... of channel c, in order
  const int parts = 1024 / CW;
  f2* p1 = col + RPS * CW;                               // [parts][CW]
  {
    const int part = t / CW, c = t - part * CW;
    if (part < parts) {
      float S = 0.f, Q = 0.f;
      for (int l = part; l < RPS; l += parts) { f2 q = col[l * CW + c]; S += q[0]; Q += q[1]; }
      p1[part * CW + c] = (f2){S, Q};
    }
  }
  __syncthreads();
  // fold 2: one wave per group: lanes stride over the (part, channel of the group) pairs in a fixed order, fp64, shuffle tree
  float* st = reinterpret_cast<float*>(p1 + parts * CW);  // [gpb][2]: mean, rstd
  {
    const int wv = t >> 6, lane = t & 63;
    if (wv < gpb) {
      double S = 0.0, Q = 0.0;
      const int npairs = parts * cpg;
      for (int q = lane; q < npairs; q += 64) {
        int part = q / cpg, c = wv * cpg + (q - part * cpg);
        f2 u = p1[part * CW + c];
        S += (double)u[0]; Q += (double)u[1];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { S += __shfl_xor(S, o, 64); Q += __shfl_xor(Q, o, 64); }
      if (lane == 0) {
        const double cnt = (double)HoWo * cpg;
        double mean = S / cnt, var = Q / cnt - mean * mean;
        if (var < 0.0) var = 0.0;
        st[2 * wv] = (float)mean; st[2 * wv + 1] = (float)(1.0 / sqrt(var + (double)eps));
        if (gn_part) { float* d = gn_part + ((long long)img * G + gs * gpb + wv) * 2; d[0] = (float)S; d[1] = (float)Q; }
      }
    }
  }
  __syncthreads();
  if (!act) return;
  float a[4], b[4];
  {
    for (int e = 0; e < 4; ++e) {
      const int g = (v * 4 + e) / cpg;
      a[e] = st[2 * g + 1] * e2f<BF>(gm[e]);
      b[e] = e2f<BF>(bt[e]) - st[2 * g] * a[e];
    }
  }
#pragma unroll
  for (int k = 0; k < RGA_MAXR; ++k) {
    const int r = rl + k * RPS;
    if (r < HoWo) {
      h4 o;
      for (int e = 0; e < 4; ++e) { float f = e2f<BF>(out[k][e]) * a[e] + b[e]; o[e] = f2e<BF>(do_silu ? silu_f(f) : f); }
      *reinterpret_cast<h4*>(z + ((long long)img * HoWo + r) * N + n) = o;
    }
  }
}
// geometry of that launch for (HoWo, N, G): groups per block, quads per row, rows per sweep, LDS bytes; false = not eligible
static bool rga_geometry(int HoWo, int N, int G, int* gpb, int* CV, int* RPS, size_t* lds) {
  if (G < 1 || N % G || N % 4) return false;
  const int cpg = N / G;
  int g = 1;
  while (g <= G && ((g * cpg) % 4 != 0 || G % g != 0)) ++g;
  if (g > G || g > 16) return false;                     // one wave per group in fold 2
  const int CW = g * cpg;
  if (CW > 256) return false;
  int cv = CW / 4, rps = 1024 / cv;
  if (rps > HoWo) rps = HoWo;
  if ((long long)rps * RGA_MAXR < HoWo) return false;
  const int parts = 1024 / CW;
  size_t bytes = ((size_t)rps * CW + (size_t)parts * CW) * 8 + (size_t)g * 8;
  if (bytes > 160 * 1024) return false;
  *gpb = g; *CV = cv; *RPS = rps; *lds = bytes;
  return true;
}

bool tfk_splitk_reduce_applies_gn(int HoWo, int N, int G) {
  int gpb, cv, rps;
  size_t lds;
  return rga_geometry(HoWo, N, G, &gpb, &cv, &rps, &lds);
}

int tfk_launch_splitk_reduce(const GemmP& p, hipStream_t st) {
  if (p.on_applied) *p.on_applied = 0;
  if (p.splitk <= 1) return TF_OK;
  const bool bf = p.bf16 != 0;
  int rg_gpb = 0, rg_cv = 0, rg_rps = 0;
  size_t rg_lds = 0;
  if (p.on_z && p.gn_part && rga_geometry(p.HoWo, p.N, p.gn_G, &rg_gpb, &rg_cv, &rg_rps, &rg_lds)) {
    static bool attr_set = false;
    if (!attr_set) {
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<float>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<half_t>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<float, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<half_t, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<half_t, false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      TF_HIP(hipFuncSetAttribute((const void*)k_splitk_reduce_gn_apply<float, true, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_set = true;
    }
    const int nimg = p.M / p.HoWo;
#define TF_RGA_LAUNCH(PT, BFV, GMV) hipLaunchKernelGGL((k_splitk_reduce_gn_apply<PT, BFV, GMV>), dim3(nimg * (p.gn_G / rg_gpb)), dim3(1024), rg_lds, st, p.y, p.on_z, (const PT*)p.partial, p.bias, p.bias_nc, \
                       p.residual, p.M, p.N, p.HoWo, p.splitk, p.bias_nc_stride, p.gn_part, p.gn_G, p.gn_cpg, rg_gpb, p.on_gamma, p.on_beta, p.on_eps, p.on_silu, rg_rps, rg_cv)
    if (p.slab_gm) {                                       // the layout the GEMM launch wrote (launch_one), never guessed here
      if (rg_gpb != 1 || (p.gn_cpg & 3)) { tf_set_error("split-K reduce: group-major slabs with %d groups per block, group width %d", rg_gpb, p.gn_cpg); return TF_E_STATE; }
      const bool pairs = ((rg_rps * rg_cv) & 1) == 0 && ((p.HoWo * rg_cv) & 1) == 0;   // 16-byte loads: every lane pair's two quads start on a 16-byte boundary
      if (bf) TF_RGA_LAUNCH(float, true, 1);
      else if (p.part16 && pairs) TF_RGA_LAUNCH(half_t, false, 2);
      else if (p.part16) TF_RGA_LAUNCH(half_t, false, 1);
      else TF_RGA_LAUNCH(float, false, 1);
    }
    else if (bf) TF_RGA_LAUNCH(float, true, 0);
    else if (p.part16) TF_RGA_LAUNCH(half_t, false, 0);
    else TF_RGA_LAUNCH(float, false, 0);
#undef TF_RGA_LAUNCH
    TF_LAUNCH_CHECK();
    if (p.on_applied) *p.on_applied = 1;
  } else if (p.gn_part) {
    const int R = p.HoWo / p.gn_chunks, nq = p.N >> 2;
    int RL = 1024 / nq;
    if (RL > R) RL = R;
    int threads = (RL * nq + 63) & ~63;
#define TF_RG_LAUNCH(PT, BFV) hipLaunchKernelGGL((k_splitk_reduce_gn<PT, BFV>), dim3(p.M / R), dim3(threads), (size_t)RL * p.N * 2 * sizeof(float), st, p.y, (const PT*)p.partial, \
                       p.bias, p.bias_nc, p.residual, p.M, p.N, p.HoWo, p.splitk, p.bias_nc_stride, p.gn_part, p.gn_G, p.gn_cpg, p.gn_chunks, R, RL)
    if (bf) TF_RG_LAUNCH(float, true);
    else if (p.part16) TF_RG_LAUNCH(half_t, false);
    else TF_RG_LAUNCH(float, false);
#undef TF_RG_LAUNCH
    TF_LAUNCH_CHECK();
  } else {
    long long nv = ((long long)p.M * p.N) >> 2;
    int grid = (int)((nv + 255) / 256);
    if (grid > 2048) grid = 2048;
    if (grid < 1) grid = 1;
#define TF_R_LAUNCH(PT, BFV) hipLaunchKernelGGL((k_splitk_reduce<PT, BFV>), dim3(grid), dim3(256), 0, st, p.y, (const PT*)p.partial, p.bias, p.bias_nc, p.residual, p.M, p.N, p.HoWo, p.splitk, p.bias_nc_stride)
    if (bf) TF_R_LAUNCH(float, true);
    else if (p.part16) TF_R_LAUNCH(half_t, false);
    else TF_R_LAUNCH(float, false);
#undef TF_R_LAUNCH
    TF_LAUNCH_CHECK();
  }
  return TF_OK;
}
