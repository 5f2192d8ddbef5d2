// FreeU (Si et al. 2023, as diffusers' apply_freeu / fourier_filter state it) on the captured SD-1.x step: in front of the channel concat of
// vision/unet.py:72 -- cat(x, saved.pop()) -- of the first two decoder stages, the skip tensor goes through a Fourier filter and the first half
// of the backbone's channels is scaled.  Own translation unit: no existing kernel's code changes.
//
// The filter at threshold 1 touches the four frequency bins (u, v) in {0, -1}^2, so it is the input plus a rank-4 correction built from seven
// real sums per (image, channel) plane -- no FFT.  With a = 2 pi i / H, b = 2 pi j / W and the per-pixel twiddles
//     t = (1, cos a, sin a, cos b, sin b, cos(a + b), sin(a + b)),
//     S_q = sum_ij x[i,j] t_q(i,j),        y[i,j] = x[i,j] + (s - 1) / (H W) * sum_q S_q t_q(i,j).
#include "common.h"
#include "../../include/tinyfusers_hip.h"

#define FU_MAX 8                         // entries of one launch (SD-1.5: the 6 skip tensors of the two stages)
#define FU_BLOCK 256
#define FU_CV 8                          // 16-byte channel vectors of one block's slab (64 channels: 128 contiguous bytes per pixel)
#define FU_PG (FU_BLOCK / FU_CV)         // pixel groups of a block: thread (pg, cv) walks the pixels pg, pg + FU_PG, ...
#define FU_Q 7                           // sums per plane
#define FU_SLAB (FU_CV * 8)              // channels of a slab
#define FU_MAX_HW 256                    // H + W of one entry: the twiddle tables are static LDS

// The whole table travels by value in the kernel arguments: nothing is uploaded, and a captured graph node owns its copy.
struct FreeuTable {
  void* dst[FU_MAX];
  const void* src[FU_MAX];
  int H[FU_MAX], W[FU_MAX];
  unsigned vpp[FU_MAX];                  // 16-byte vectors per pixel (C / 8)
  unsigned slabs[FU_MAX];                // ceil(vpp / FU_CV)
  unsigned sidx[FU_MAX];                 // index into scales
  unsigned first[FU_MAX + 1];            // prefix sum of the blocks: entry i owns [first[i], first[i+1]), one block per (image, slab)
  int n;
};

// One block = one image's slab of up to 64 channels of one entry: lanes run along the channels (cv, one 16-byte vector each), the block's 32
// pixel groups split the plane's pixels.  Pass 1: every thread's 7 x 8 fp32 partial sums over its pixels, combined through LDS in ascending
// pixel-group order (no atomics: a replay computes what the eager launch computes, bit for bit).  Pass 2 re-reads the slab (L2) and writes
// round16(fmaf(g, sum_q S_q t_q, x)).  s == 1 is a uniform branch that copies the source's bits (0 * inf would be NaN) and returns at once when
// dst is src.  dst may alias src: a block reads its slab, synchronises, and then every element is read and written by the same thread.
template <bool BF>
__global__ void __launch_bounds__(FU_BLOCK) k_freeu_skip(const FreeuTable t, const float* __restrict__ scales) {
  __shared__ __attribute__((aligned(16))) float red[FU_PG * FU_Q * FU_SLAB];      // [pg][q][channel of the slab]: 56 KiB
  __shared__ float tot[FU_Q * FU_SLAB];
  __shared__ float tw[2 * FU_MAX_HW];                                              // cos | sin of 2 pi i / H (i < H), then of 2 pi j / W (j < W)
  const unsigned blk = blockIdx.x;
  void* dst = t.dst[0];
  const void* src = t.src[0];
  int H = t.H[0], W = t.W[0];
  unsigned vpp = t.vpp[0], slabs = t.slabs[0], sidx = t.sidx[0], first = 0;
#pragma unroll
  for (int i = 1; i < FU_MAX; ++i) {
    if (i < t.n && blk >= t.first[i]) {
      dst = t.dst[i]; src = t.src[i]; H = t.H[i]; W = t.W[i]; vpp = t.vpp[i]; slabs = t.slabs[i]; sidx = t.sidx[i]; first = t.first[i];
    }
  }
  const float s = scales[sidx];
  const unsigned r = blk - first;
  const unsigned img = r / slabs, slab = r - img * slabs;
  const int cv = threadIdx.x & (FU_CV - 1), pg = threadIdx.x / FU_CV;
  const unsigned v = slab * FU_CV + cv;                  // this lane's vector within a pixel
  const bool live = v < vpp;
  const int HW = H * W;
  const h8* x = reinterpret_cast<const h8*>(src) + (size_t)img * HW * vpp + v;
  h8* y = reinterpret_cast<h8*>(dst) + (size_t)img * HW * vpp + v;
  if (s == 1.0f) {
    if (dst == src || !live) return;
    for (int p = pg; p < HW; p += FU_PG) y[(size_t)p * vpp] = x[(size_t)p * vpp];
    return;
  }
  for (int k = threadIdx.x; k < H + W; k += FU_BLOCK) {
    const double a = k < H ? 2.0 * k / H : 2.0 * (k - H) / W;
    double sn, cs;
    sincospi(a, &sn, &cs);
    tw[2 * k] = (float)cs; tw[2 * k + 1] = (float)sn;
  }
  __syncthreads();
  float acc[FU_Q][8];
#pragma unroll
  for (int q = 0; q < FU_Q; ++q)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[q][k] = 0.0f;
  if (live) {
    for (int p = pg; p < HW; p += FU_PG) {
      const int i = p / W, j = p - i * W;
      const float ci = tw[2 * i], si = tw[2 * i + 1], cj = tw[2 * (H + j)], sj = tw[2 * (H + j) + 1];
      const float cc = fmaf(ci, cj, -(si * sj)), ss = fmaf(si, cj, ci * sj);
      const h8 xv = x[(size_t)p * vpp];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float f = e2f<BF>(xv[k]);
        acc[0][k] += f;
        acc[1][k] = fmaf(f, ci, acc[1][k]); acc[2][k] = fmaf(f, si, acc[2][k]);
        acc[3][k] = fmaf(f, cj, acc[3][k]); acc[4][k] = fmaf(f, sj, acc[4][k]);
        acc[5][k] = fmaf(f, cc, acc[5][k]); acc[6][k] = fmaf(f, ss, acc[6][k]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < FU_Q; ++q) {
    f4* w4 = reinterpret_cast<f4*>(&red[(pg * FU_Q + q) * FU_SLAB + cv * 8]);
    w4[0] = f4{acc[q][0], acc[q][1], acc[q][2], acc[q][3]};
    w4[1] = f4{acc[q][4], acc[q][5], acc[q][6], acc[q][7]};
  }
  __syncthreads();
  for (int o = threadIdx.x; o < FU_Q * FU_SLAB; o += FU_BLOCK) {
    float a = red[o];
#pragma unroll 8
    for (int g = 1; g < FU_PG; ++g) a += red[g * (FU_Q * FU_SLAB) + o];
    tot[o] = a;
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int q = 0; q < FU_Q; ++q)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[q][k] = tot[q * FU_SLAB + cv * 8 + k];
  const float g = (s - 1.0f) / (float)HW;
  for (int p = pg; p < HW; p += FU_PG) {
    const int i = p / W, j = p - i * W;
    const float ci = tw[2 * i], si = tw[2 * i + 1], cj = tw[2 * (H + j)], sj = tw[2 * (H + j) + 1];
    const float cc = fmaf(ci, cj, -(si * sj)), ss = fmaf(si, cj, ci * sj);
    const h8 xv = x[(size_t)p * vpp];
    h8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float c = acc[0][k];
      c = fmaf(acc[1][k], ci, c); c = fmaf(acc[2][k], si, c);
      c = fmaf(acc[3][k], cj, c); c = fmaf(acc[4][k], sj, c);
      c = fmaf(acc[5][k], cc, c); c = fmaf(acc[6][k], ss, c);
      o[k] = f2e<BF>(fmaf(g, c, e2f<BF>(xv[k])));
    }
    y[(size_t)p * vpp] = o;
  }
}

// dst[r, c] = round16(b * src[r, c]) for c < C / 2 (one fp32 multiply, one rounding); the second half of the channels is copied when COPY
// (dst != src) and not touched otherwise.  b == 1 copies the bits.  vpr: 16-byte vectors per row the launch visits (C / 8 | C / 16)
template <bool BF, bool COPY>
__global__ void __launch_bounds__(EW_BLOCK) k_freeu_backbone(h8* dst, const h8* src, long long rows, int C,
                                                             const float* __restrict__ scales, int sidx) {
  const float b = scales[sidx];
  if (!COPY && b == 1.0f) return;
  const int half = C >> 4, vpr = COPY ? C >> 3 : half;
  const long long nv = rows * vpr, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; i < nv; i += gs) {
    const long long r = i / vpr;
    const int c = (int)(i - r * vpr);
    const long long at = r * (C >> 3) + c;
    h8 v = src[at];
    if (c < half && b != 1.0f) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = f2e<BF>(b * e2f<BF>(v[k]));
    }
    dst[at] = v;
  }
}

extern "C" {

int tf_freeu_skip_16(int dtype, const void* table, int n_entries, const void* scales_f32, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_freeu_skip_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(table && scales_f32 && n_entries >= 1 && n_entries <= FU_MAX, "tf_freeu_skip_16: bad arguments (n_entries=%d, 1..%d)", n_entries, FU_MAX);
  TF_REQUIRE(((uintptr_t)scales_f32 & 3) == 0, "tf_freeu_skip_16: scales must be 4-byte aligned");
  const tfFreeuEntry* in = (const tfFreeuEntry*)table;
  FreeuTable t = {};
  t.n = n_entries;
  long long first = 0;
  for (int i = 0; i < n_entries; ++i) {
    const tfFreeuEntry& e = in[i];
    TF_REQUIRE(e.dst && e.src, "tf_freeu_skip_16: entry %d holds a null pointer", i);
    TF_REQUIRE(e.B >= 1 && e.C >= 8 && e.C % 8 == 0, "tf_freeu_skip_16: entry %d has B=%d, C=%d (B >= 1, C a positive multiple of 8)", i, e.B, e.C);
    TF_REQUIRE(e.H >= 2 && e.W >= 2, "tf_freeu_skip_16: entry %d has H=%d, W=%d (the filter's 2 x 2 box needs H >= 2 and W >= 2)", i, e.H, e.W);
    TF_REQUIRE(e.H + e.W <= FU_MAX_HW, "tf_freeu_skip_16: entry %d has H + W = %d (at most %d)", i, e.H + e.W, FU_MAX_HW);
    TF_REQUIRE((((uintptr_t)e.dst | (uintptr_t)e.src) & 15) == 0, "tf_freeu_skip_16: entry %d is not 16-byte aligned", i);
    TF_REQUIRE(e.scale_index >= 0, "tf_freeu_skip_16: entry %d has scale_index=%d", i, e.scale_index);
    t.dst[i] = e.dst; t.src[i] = e.src; t.H[i] = e.H; t.W[i] = e.W;
    t.vpp[i] = (unsigned)(e.C / 8);
    t.slabs[i] = (t.vpp[i] + FU_CV - 1) / FU_CV;
    t.sidx[i] = (unsigned)e.scale_index;
    t.first[i] = (unsigned)first;
    first += (long long)e.B * t.slabs[i];
    TF_REQUIRE(first < (1LL << 31), "tf_freeu_skip_16: %lld blocks exceed one launch (2^31)", first);
  }
  for (int i = n_entries; i <= FU_MAX; ++i) t.first[i] = (unsigned)first;
  const bool bf = dtype == TF_DTYPE_BF16;
  hipLaunchKernelGGL(bf ? k_freeu_skip<true> : k_freeu_skip<false>, dim3((unsigned)first), dim3(FU_BLOCK), 0, tf_hs(s), t, (const float*)scales_f32);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_freeu_backbone_16(int dtype, void* dst, const void* src, long long rows, int C, const void* scales_f32, int scale_index, tfStream_t s) {
  TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, "tf_freeu_backbone_16: dtype=%d (0 = float16, 1 = bfloat16)", dtype);
  TF_REQUIRE(dst && src && scales_f32 && rows >= 0 && scale_index >= 0, "tf_freeu_backbone_16: bad arguments (rows=%lld, scale_index=%d)", rows, scale_index);
  TF_REQUIRE(C >= 16 && C % 16 == 0, "tf_freeu_backbone_16: C=%d (a positive multiple of 16: each half of the channels is whole 16-byte vectors)", C);
  TF_REQUIRE((((uintptr_t)dst | (uintptr_t)src) & 15) == 0 && ((uintptr_t)scales_f32 & 3) == 0, "tf_freeu_backbone_16: dst and src must be 16-byte aligned, scales 4-byte");
  if (rows == 0) return TF_OK;
  const bool bf = dtype == TF_DTYPE_BF16, copy = dst != src;
  const int grid = ew_grid(rows * (copy ? C / 8 : C / 16));
  const float* sc = (const float*)scales_f32;
  auto kern = copy ? (bf ? k_freeu_backbone<true, true> : k_freeu_backbone<false, true>) : (bf ? k_freeu_backbone<true, false> : k_freeu_backbone<false, false>);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(EW_BLOCK), 0, tf_hs(s), (h8*)dst, (const h8*)src, rows, C, sc, scale_index);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
