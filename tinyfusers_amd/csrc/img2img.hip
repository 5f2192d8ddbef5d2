// The edges of the VAE encoder (vae/vae.py:12-15: uint8 image -> encoder input, means -> latent, the inverse of variants/sd.py:48-54) for
// image-to-image, masked inpainting and the concat-conditioned checkpoints: the image as the encoder reads it, plain or with the repainted
// region greyed out, and the encoder's means as a clean latent or as channels of a conditioning buffer.  What happens to that latent
// afterwards (the noising to a start level, the sampler update and its blend) is csrc/sampler.hip.
#include "common.h"
#include "../../include/tinyfusers_hip.h"

// (2u - 255) / 255 = u / 127.5 - 1: one correctly rounded fp32 division of two exact integers, then fp16 -- for every u in 0..255 the fp16
// of the exact value (tests/test_img2img_host.py checks all 256).  tf_image_to_u8 maps it back to u.
__device__ __forceinline__ half_t u8_to_unit(unsigned u) { return (half_t)((float)(2 * (int)u - 255) / 255.0f); }

// n elements, 4 per thread: uchar4 in, h4 out when VEC (n % 4 == 0 and both pointers aligned to their vector)
template <bool VEC>
__global__ void __launch_bounds__(EW_BLOCK) k_image_from_u8(half_t* __restrict__ out, const unsigned char* __restrict__ in, long long n) {
  const long long nq = (n + 3) >> 2, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; t < nq; t += gs) {
    if (VEC) {
      const uchar4 v = reinterpret_cast<const uchar4*>(in)[t];
      h4 o;
      o.x = u8_to_unit(v.x); o.y = u8_to_unit(v.y); o.z = u8_to_unit(v.z); o.w = u8_to_unit(v.w);
      reinterpret_cast<h4*>(out)[t] = o;
    } else {
      for (long long i = 4 * t; i < 4 * t + 4 && i < n; ++i) out[i] = u8_to_unit(in[i]);
    }
  }
}

// image (P, 3) uint8, mask (P) uint8 -> out (P, 3) fp16 = u / 127.5 - 1 where the pixel's mask byte is 0, +0 where it is not (the masked
// image of the inpainting model: the repainted region is grey, 0 in [-1, 1]).  One thread per element
__global__ void __launch_bounds__(EW_BLOCK) k_image_from_u8_masked(half_t* __restrict__ out, const unsigned char* __restrict__ in,
                                                                   const unsigned char* __restrict__ mask, long long n) {
  const long long gs = (long long)gridDim.x * EW_BLOCK;
  for (long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; i < n; i += gs) out[i] = mask[i / 3] ? (half_t)0.0f : u8_to_unit(in[i]);
}

// means (B, HW, 4) fp16 (NHWC, 4 channels) -> channels [c_off, c_off + 4) of cond (B, Ct, HW) fp32 NCHW = scale * means.  One thread per
// pixel: one 8-byte load, four stores
__global__ void __launch_bounds__(EW_BLOCK) k_means_to_cond(float* __restrict__ cond, const h4* __restrict__ means, int B, int HW, float scale, int c_off, int Ct) {
  const long long total = (long long)B * HW, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; t < total; t += gs) {
    const int b = (int)(t / HW), hw = (int)(t - (long long)b * HW);
    const h4 m = means[t];
    float* o = cond + ((long long)b * Ct + c_off) * HW + hw;
    o[0] = scale * (float)m.x;
    o[HW] = scale * (float)m.y;
    o[2 * (long long)HW] = scale * (float)m.z;
    o[3 * (long long)HW] = scale * (float)m.w;
  }
}

extern "C" {

int tf_image_from_u8_f16(void* out, const void* x, long long n, tfStream_t s) {
  TF_REQUIRE(out && x && n >= 0, "tf_image_from_u8_f16: bad arguments (n=%lld)", n);
  if (n == 0) return TF_OK;
  const bool vec = n % 4 == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)x & 3) == 0;
  const int grid = ew_grid((n + 3) >> 2);
  if (vec)
    hipLaunchKernelGGL(k_image_from_u8<true>, dim3(grid), dim3(EW_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)x, n);
  else
    hipLaunchKernelGGL(k_image_from_u8<false>, dim3(grid), dim3(EW_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)x, n);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_image_from_u8_masked_f16(void* out, const void* image_u8, const void* mask_u8, int B, int H, int W, tfStream_t s) {
  TF_REQUIRE(out && image_u8 && mask_u8 && B >= 0 && H >= 0 && W >= 0, "tf_image_from_u8_masked_f16: bad arguments (B=%d H=%d W=%d)", B, H, W);
  TF_REQUIRE(((uintptr_t)out & 1) == 0, "tf_image_from_u8_masked_f16: out must be 2-byte aligned");
  const long long n = 3LL * B * H * W;
  if (n == 0) return TF_OK;
  hipLaunchKernelGGL(k_image_from_u8_masked, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)image_u8,
                     (const unsigned char*)mask_u8, n);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

// x0 (B,4,HW) fp32 NCHW = 0.18215 means: k_means_to_cond onto all 4 channels of a 4-channel buffer (the same fp32 product)
int tf_means_to_latent_f32(void* x0, const void* means, int B, int H, int W, tfStream_t s) {
  TF_REQUIRE(x0 && means && B >= 0 && H >= 0 && W >= 0, "tf_means_to_latent_f32: bad arguments (B=%d H=%d W=%d)", B, H, W);
  TF_REQUIRE(((uintptr_t)means & 7) == 0, "tf_means_to_latent_f32: means must be 8-byte aligned (one 4-channel fp16 pixel)");
  const long long total = (long long)B * H * W;
  TF_REQUIRE((long long)H * W < (1LL << 31), "tf_means_to_latent_f32: %lld pixels per image", (long long)H * W);
  if (total == 0) return TF_OK;
  hipLaunchKernelGGL(k_means_to_cond, dim3(ew_grid(total)), dim3(EW_BLOCK), 0, tf_hs(s), (float*)x0, (const h4*)means, B, H * W, 0.18215f, 0, 4);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_means_to_cond_f32(void* cond, const void* means, int B, int H, int W, float scale, int c_off, int c_total, tfStream_t s) {
  TF_REQUIRE(cond && means && B >= 0 && H >= 0 && W >= 0, "tf_means_to_cond_f32: bad arguments (B=%d H=%d W=%d)", B, H, W);
  TF_REQUIRE(c_off >= 0 && c_total >= 4 && c_off <= c_total - 4, "tf_means_to_cond_f32: channels [%d, %d) do not lie in the %d of the buffer", c_off, c_off + 4, c_total);
  TF_REQUIRE(((uintptr_t)means & 7) == 0, "tf_means_to_cond_f32: means must be 8-byte aligned (one 4-channel fp16 pixel)");
  TF_REQUIRE((long long)H * W < (1LL << 31), "tf_means_to_cond_f32: %lld pixels per image", (long long)H * W);
  const long long total = (long long)B * H * W;
  if (total == 0) return TF_OK;
  hipLaunchKernelGGL(k_means_to_cond, dim3(ew_grid(total)), dim3(EW_BLOCK), 0, tf_hs(s), (float*)cond, (const h4*)means, B, H * W, scale, c_off, c_total);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
