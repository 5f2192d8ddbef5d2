// The three kernels a CLIP ViT image tower needs beyond the text tower's (vae/clip_vision.py): the input edge (uint8 image -> normalised
// patch matrix, the A operand of the patch-embedding GEMM), the token assembly (class row | patch rows, + position rows, pre-LayerNorm) and the
// exact (erf) GELU.  All three are memory-bound: 16 B per lane on every 16-bit tensor, fp32 arithmetic, plain stores, no atomics -- a graph
// replay is bit-identical to the eager launch.  The uint8 image is read by bytes: with (ky, kx, c) columns a patch row is 3P contiguous
// bytes at an offset that is a multiple of 3P (42 for P = 14), never of 16; the image is a third of the launch's traffic and adjacent lanes
// read adjacent 8-byte runs.
#include <math.h>

#include "common.h"
#include "../../include/tinyfusers_hip.h"

#define VIT_BLOCK EW_BLOCK     // (k_vit_patchify and k_gelu_erf launch on ew_grid)
#define VIT_LN_MAXV 5          // k_layer_norm's register form (csrc/norm.hip): a lane holds <= 5 vectors of 8, D <= 2560

struct Norm3 { float scale[3], shift[3]; };

// out (B (S/P)^2, Kpad): row (b, py, px), column ky 3P + kx 3 + c = fmaf(u8, scale[c], shift[c]) of pixel (py P + ky, px P + kx), channel c;
// columns >= 3 P^2 are zero.  One thread per 8 columns.
template <typename T>
__global__ void __launch_bounds__(VIT_BLOCK) k_vit_patchify(T* __restrict__ out, const unsigned char* __restrict__ img, int S, int P, int Kpad,
                                                            long long nvec, Norm3 nm) {
  typedef T T8 __attribute__((ext_vector_type(8)));
  const int G = S / P, KV = Kpad >> 3, run = 3 * P, K = run * P;
  const long long stride = (long long)gridDim.x * VIT_BLOCK;
  for (long long i = (long long)blockIdx.x * VIT_BLOCK + threadIdx.x; i < nvec; i += stride) {
    const long long row = i / KV;
    const int col0 = (int)(i - row * KV) * 8;
    const int px = (int)(row % G), py = (int)((row / G) % G);
    const long long b = row / ((long long)G * G);
    const unsigned char* base = img + ((b * S + (long long)py * P) * S + (long long)px * P) * 3;
    T8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = col0 + j;
      float f = 0.f;
      if (col < K) {
        const int ky = col / run, r = col - ky * run, c = r % 3;
        f = fmaf((float)base[(long long)ky * S * 3 + r], nm.scale[c], nm.shift[c]);
      }
      o[j] = (T)f;
    }
    *reinterpret_cast<T8*>(out + i * 8) = o;
  }
}

// out (B, T, D) = LayerNorm(row + pos[t]) with row = class_emb for t = 0, patch_out[b, t - 1] beyond; the sum stays fp32.  One wave per row,
// the row in registers (k_layer_norm<64>'s two-pass form).
template <typename T>
__global__ void __launch_bounds__(VIT_BLOCK) k_vit_embed_ln(T* __restrict__ out, const T* __restrict__ patch_out, const T* __restrict__ class_emb,
                                                            const T* __restrict__ pos, const T* __restrict__ gamma, const T* __restrict__ beta,
                                                            int rows, int Tn, int D, float eps) {
  typedef T T8 __attribute__((ext_vector_type(8)));
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + w;
  if (row >= rows) return;                               // (wave-uniform: the shuffles below run on whole waves)
  const int b = row / Tn, t = row - b * Tn;
  const T* src = t == 0 ? class_emb : patch_out + ((long long)b * (Tn - 1) + (t - 1)) * D;
  const T* pr = pos + (long long)t * D;
  const int CV = D >> 3;
  float v[VIT_LN_MAXV][8];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VIT_LN_MAXV; ++i) {
    const int cv = l + 64 * i;
    if (cv < CV) {
      const T8 a = *reinterpret_cast<const T8*>(src + cv * 8), p = *reinterpret_cast<const T8*>(pr + cv * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[i][j] = (float)a[j] + (float)p[j]; s += v[i][j]; }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VIT_LN_MAXV; ++i) {
    if (l + 64 * i < CV) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; q += d * d; }
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) q += __shfl_xor(q, o, 64);
  const float rstd = rsqrtf(q / (float)D + eps);
  T* yr = out + (long long)row * D;
#pragma unroll
  for (int i = 0; i < VIT_LN_MAXV; ++i) {
    const int cv = l + 64 * i;
    if (cv < CV) {
      const T8 gm = *reinterpret_cast<const T8*>(gamma + cv * 8), bt = *reinterpret_cast<const T8*>(beta + cv * 8);
      T8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (T)((v[i][j] - mean) * rstd * (float)gm[j] + (float)bt[j]);
      *reinterpret_cast<T8*>(yr + cv * 8) = o;
    }
  }
}

// exact GELU as 0.5 x erfc(-x / sqrt 2): 1 + erf(x / sqrt 2) cancels in the negative tail, erfc does not
__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * erfcf(-x * 0.70710678118654752440f); }

template <typename T>
__global__ void __launch_bounds__(VIT_BLOCK) k_gelu_erf(T* y, const T* x, long long n) {       // (y may be x: no __restrict__)
  typedef T T8 __attribute__((ext_vector_type(8)));
  const long long nvec = n >> 3, stride = (long long)gridDim.x * VIT_BLOCK;
  for (long long i = (long long)blockIdx.x * VIT_BLOCK + threadIdx.x; i < nvec; i += stride) {
    const T8 v = *reinterpret_cast<const T8*>(x + i * 8);
    T8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (T)gelu_erf_f((float)v[j]);
    *reinterpret_cast<T8*>(y + i * 8) = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 7)) {
    const long long i = (nvec << 3) + threadIdx.x;
    y[i] = (T)gelu_erf_f((float)x[i]);
  }
}

#define VIT_DTYPE(name) TF_REQUIRE(dtype == TF_DTYPE_F16 || dtype == TF_DTYPE_BF16, name ": dtype=%d (0 = float16, 1 = bfloat16)", dtype)
#define VIT_ALIGNED16(p) (((uintptr_t)(p) & 15) == 0)

extern "C" {

int tf_vit_patchify_u8_16(int dtype, void* out, const void* image_u8, int B, int S, int P, int Kpad, const float* scale3, const float* shift3,
                          tfStream_t s) {
  VIT_DTYPE("tf_vit_patchify_u8_16");
  TF_REQUIRE(out && image_u8 && scale3 && shift3, "tf_vit_patchify_u8_16: null argument");
  TF_REQUIRE(B >= 0 && S >= 1 && P >= 1 && S % P == 0, "tf_vit_patchify_u8_16: B=%d S=%d P=%d (S must be a positive multiple of P)", B, S, P);
  TF_REQUIRE(P <= 64 && S <= 16384, "tf_vit_patchify_u8_16: P=%d S=%d out of range (P <= 64, S <= 16384)", P, S);
  TF_REQUIRE(Kpad % 8 == 0 && Kpad >= 3 * P * P, "tf_vit_patchify_u8_16: Kpad=%d must be a multiple of 8 and >= 3 P^2 = %d", Kpad, 3 * P * P);
  TF_REQUIRE(VIT_ALIGNED16(out), "tf_vit_patchify_u8_16: out must be 16-byte aligned");
  for (int c = 0; c < 3; ++c) TF_REQUIRE(isfinite(scale3[c]) && isfinite(shift3[c]), "tf_vit_patchify_u8_16: scale3 / shift3 must be finite");
  if (B == 0) return TF_OK;
  Norm3 nm;
  for (int c = 0; c < 3; ++c) { nm.scale[c] = scale3[c]; nm.shift[c] = shift3[c]; }
  const long long nvec = (long long)B * (S / P) * (S / P) * (Kpad >> 3);
  TfProfScope prof_(TF_PROF_FAM_VIT_ELEMENTWISE, (double)B * S * S * 3.0 + (double)nvec * 16.0, tf_hs(s));    // the image in, the patch matrix out
  if (dtype == TF_DTYPE_BF16)
    hipLaunchKernelGGL(k_vit_patchify<bf16_t>, dim3(ew_grid(nvec)), dim3(VIT_BLOCK), 0, tf_hs(s), (bf16_t*)out, (const unsigned char*)image_u8, S, P, Kpad, nvec, nm);
  else
    hipLaunchKernelGGL(k_vit_patchify<half_t>, dim3(ew_grid(nvec)), dim3(VIT_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)image_u8, S, P, Kpad, nvec, nm);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_vit_embed_ln_16(int dtype, void* out, const void* patch_out, const void* class_emb, const void* pos_emb, const void* gamma, const void* beta,
                       int B, int T, int D, float eps, tfStream_t s) {
  VIT_DTYPE("tf_vit_embed_ln_16");
  TF_REQUIRE(out && class_emb && pos_emb && gamma && beta && (patch_out || T == 1), "tf_vit_embed_ln_16: null tensor");
  TF_REQUIRE(B >= 0 && T >= 1 && (long long)B * T <= 0x7fffffffLL / 4, "tf_vit_embed_ln_16: B=%d T=%d out of range", B, T);
  TF_REQUIRE(D > 0 && D % 8 == 0 && D <= 64 * 8 * VIT_LN_MAXV, "tf_vit_embed_ln_16: D=%d must be a multiple of 8 and <= %d (tf_layer_norm's register form)", D,
             64 * 8 * VIT_LN_MAXV);
  TF_REQUIRE(eps > 0.f && isfinite(eps), "tf_vit_embed_ln_16: eps=%g", (double)eps);
  TF_REQUIRE(VIT_ALIGNED16(out) && VIT_ALIGNED16(patch_out) && VIT_ALIGNED16(class_emb) && VIT_ALIGNED16(pos_emb) && VIT_ALIGNED16(gamma) && VIT_ALIGNED16(beta),
             "tf_vit_embed_ln_16: every tensor must be 16-byte aligned");
  if (B == 0) return TF_OK;
  const int rows = B * T;
  TfProfScope prof_(TF_PROF_FAM_LAYER_NORM, (double)rows * D * 6.0, tf_hs(s));          // patch row + position row in, the normalised row out
  if (dtype == TF_DTYPE_BF16)
    hipLaunchKernelGGL(k_vit_embed_ln<bf16_t>, dim3(ceil_div(rows, 4)), dim3(VIT_BLOCK), 0, tf_hs(s), (bf16_t*)out, (const bf16_t*)patch_out, (const bf16_t*)class_emb,
                       (const bf16_t*)pos_emb, (const bf16_t*)gamma, (const bf16_t*)beta, rows, T, D, eps);
  else
    hipLaunchKernelGGL(k_vit_embed_ln<half_t>, dim3(ceil_div(rows, 4)), dim3(VIT_BLOCK), 0, tf_hs(s), (half_t*)out, (const half_t*)patch_out, (const half_t*)class_emb,
                       (const half_t*)pos_emb, (const half_t*)gamma, (const half_t*)beta, rows, T, D, eps);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_gelu_erf_16(int dtype, void* y, const void* x, long long n, tfStream_t s) {
  VIT_DTYPE("tf_gelu_erf_16");
  TF_REQUIRE(y && x && n >= 0, "tf_gelu_erf_16: bad arguments (n=%lld)", n);
  TF_REQUIRE(VIT_ALIGNED16(y) && VIT_ALIGNED16(x), "tf_gelu_erf_16: y and x must be 16-byte aligned");
  if (n == 0) return TF_OK;
  TfProfScope prof_(TF_PROF_FAM_VIT_ELEMENTWISE, (double)n * 4.0, tf_hs(s));
  if (dtype == TF_DTYPE_BF16) hipLaunchKernelGGL(k_gelu_erf<bf16_t>, dim3(ew_grid(n >> 3)), dim3(VIT_BLOCK), 0, tf_hs(s), (bf16_t*)y, (const bf16_t*)x, n);
  else hipLaunchKernelGGL(k_gelu_erf<half_t>, dim3(ew_grid(n >> 3)), dim3(VIT_BLOCK), 0, tf_hs(s), (half_t*)y, (const half_t*)x, n);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
