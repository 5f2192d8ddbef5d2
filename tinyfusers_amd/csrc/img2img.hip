// Image-to-image and masked inpainting on the sampler of csrc/sampler.hip: the edges of the VAE encoder (vae/vae.py:12-15: uint8 image ->
// encoder input, means -> latent, the inverse of variants/sd.py:48-54), the noising of a clean latent to the start level of a truncated
// schedule (SDEdit), and the latent-blend inpainting update.  Own translation unit: no existing kernel's code changes.
//
// Philox tags (philox.h; counter = (q, global image index, step, tag)):
//   0  the initial latent: tf_randn_f32 and tf_noise_to_level_f32 (step 0) draw the same z, so an img2img image and a text-to-image image of
//      one seed share their noise
//   1  the ancestral noise of schedule row `step` (k_cfg_sampler, k_cfg_sampler_masked)
//   2  the noise that puts the known region of an inpainting step on its trajectory, step = the schedule row
#include "common.h"
#include "philox.h"
#include "../../include/tinyfusers_hip.h"

#define I2I_BLOCK 256

static inline int i2i_grid(long long nthreads) {
  long long g = (nthreads + I2I_BLOCK - 1) / I2I_BLOCK;
  if (g > 256 * 8) g = 256 * 8;   // grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// (2u - 255) / 255 = u / 127.5 - 1: one correctly rounded fp32 division of two exact integers, then fp16 -- for every u in 0..255 the fp16
// of the exact value (tests/test_img2img_host.py checks all 256).  tf_image_to_u8 maps it back to u.
__device__ __forceinline__ half_t u8_to_unit(unsigned u) { return (half_t)((float)(2 * (int)u - 255) / 255.0f); }

// n elements, 4 per thread: uchar4 in, h4 out when VEC (n % 4 == 0 and both pointers aligned to their vector)
template <bool VEC>
__global__ void __launch_bounds__(I2I_BLOCK) k_image_from_u8(half_t* __restrict__ out, const unsigned char* __restrict__ in, long long n) {
  const long long nq = (n + 3) >> 2, gs = (long long)gridDim.x * I2I_BLOCK;
  for (long long t = (long long)blockIdx.x * I2I_BLOCK + threadIdx.x; t < nq; t += gs) {
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

// means (B, HW, 4) fp16 (NHWC, 4 channels) -> x0 (B, 4, HW) fp32 NCHW, x0 = 0.18215 means.  One thread per pixel: one 8-byte load, four stores
__global__ void __launch_bounds__(I2I_BLOCK) k_means_to_latent(float* __restrict__ x0, const h4* __restrict__ means, int B, int HW) {
  const long long total = (long long)B * HW, gs = (long long)gridDim.x * I2I_BLOCK;
  for (long long t = (long long)blockIdx.x * I2I_BLOCK + threadIdx.x; t < total; t += gs) {
    const int b = (int)(t / HW), hw = (int)(t - (long long)b * HW);
    const h4 m = means[t];
    float* o = x0 + (long long)b * 4 * HW + hw;
    o[0] = 0.18215f * (float)m.x;
    o[HW] = 0.18215f * (float)m.y;
    o[2 * (long long)HW] = 0.18215f * (float)m.z;
    o[3 * (long long)HW] = 0.18215f * (float)m.w;
  }
}

// out = sqrt(a) x0 + sqrt(1 - a) z, z the tag-0 normal of global image image0 + k at step 0.  out may alias x0 (each element is read, then
// written, by the same thread).  One thread per Philox counter: 4 NCHW elements
__global__ void __launch_bounds__(I2I_BLOCK) k_noise_to_level(float* out, const float* x0, long long n_img, int images, float a, u32 k0, u32 k1, u32 image0) {
  const float sa = sqrtf(a), sn = sqrtf(1.0f - a);
  const long long nq = (n_img + 3) >> 2, total = nq * images, gs = (long long)gridDim.x * I2I_BLOCK;
  for (long long t = (long long)blockIdx.x * I2I_BLOCK + threadIdx.x; t < total; t += gs) {
    const int k = (int)(t / nq);
    const long long q = t - (long long)k * nq;
    float z[4];
    normal4(k0, k1, (u32)q, image0 + (u32)k, 0u, 0u, z);
    const long long base = (long long)k * n_img + 4 * q, left = n_img - 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < left) out[base + j] = sa * x0[base + j] + sn * z[j];
  }
}

// k_cfg_sampler (csrc/sampler.hip) followed by the inpainting blend.  x' is computed exactly as there, in the same expression order:
// e = e_u + g (e_c - e_u); x0 = (x - sqrt(1-a_t) e) / sqrt(a_t); x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z (tag 1); x0_prev <- x0.  Then
// x' <- m x' + (1 - m) (sqrt(a_s) x0_init + sqrt(1 - a_s) z2), a_s = params[2] (the a_prev of tf_set_sampler_params), z2 the tag-2 normal at
// step = row.  m = 1 leaves x' as it is (1 x' + 0); m = 0 at the last step (a_s = 1) gives x0_init exactly.  mask (B, 1, H, W) fp32.
template <typename T>
__global__ void __launch_bounds__(I2I_BLOCK) k_cfg_sampler_masked(float* __restrict__ lat, const T* __restrict__ eps2, float* __restrict__ x0h,
                                                                 const float* __restrict__ params, const float* __restrict__ coeffs, int rows,
                                                                 const float* __restrict__ x0i, const float* __restrict__ mask, int B, int C, int HW) {
  const u32* w = reinterpret_cast<const u32*>(params);
  const float a_t = params[1], a_s = params[2], g = params[3];
  u32 row = w[4];
  if (row >= (u32)rows) row = (u32)rows - 1;                     // memory safety only: the host entry writes a row of the schedule
  const u32 k0 = w[5], k1 = w[6], image0 = w[7];
  const float cx = coeffs[4 * row], c0 = coeffs[4 * row + 1], c1 = coeffs[4 * row + 2], cn = coeffs[4 * row + 3];
  const float s1 = sqrtf(1.0f - a_t), r = sqrtf(a_t);
  const float ra = sqrtf(a_s), rn = sqrtf(1.0f - a_s);
  const long long n_img = (long long)C * HW, n = n_img * B, nq = (n_img + 3) >> 2, total = nq * B, gs = (long long)gridDim.x * I2I_BLOCK;
  for (long long t = (long long)blockIdx.x * I2I_BLOCK + threadIdx.x; t < total; t += gs) {
    const int b = (int)(t / nq);
    const long long q = t - (long long)b * nq;
    float z[4] = {0.f, 0.f, 0.f, 0.f}, z2[4];
    if (cn != 0.f) normal4(k0, k1, (u32)q, image0 + (u32)b, row, 1u, z);
    normal4(k0, k1, (u32)q, image0 + (u32)b, row, 2u, z2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * q + j;
      if (e >= n_img) break;
      const int c = (int)(e / HW), hw = (int)(e - (long long)c * HW);
      const long long i = (long long)b * n_img + e, je = ((long long)b * HW + hw) * C + c;
      const float eu = (float)eps2[je], ec = (float)eps2[n + je];
      const float ee = eu + g * (ec - eu);
      const float x = lat[i];
      const float x0 = (x - s1 * ee) / r;
      float xn = cx * x + c0 * x0;
      if (c1 != 0.f) xn += c1 * x0h[i];
      if (cn != 0.f) xn += cn * z[j];
      const float m = mask[(long long)b * HW + hw];
      const float kn = ra * x0i[i] + rn * z2[j];
      lat[i] = m * xn + (1.0f - m) * kn;
      x0h[i] = x0;
    }
  }
}

template <typename T>
static int cfg_sampler_step_masked(const char* name, void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows,
                                   const void* x0_init, const void* mask, int B, int C, int H, int W, tfStream_t s) {
  TF_REQUIRE(latent && eps2 && x0_hist && params && coeffs && x0_init && mask && rows >= 1 && B > 0 && C > 0 && H > 0 && W > 0,
             "%s: bad arguments (rows=%d B=%d C=%d H=%d W=%d)", name, rows, B, C, H, W);
  const long long n_img = (long long)C * H * W;
  TF_REQUIRE(n_img <= (1LL << 32), "%s: %lld elements per image exceed the 2^32 Philox counters of an image", name, n_img);
  hipLaunchKernelGGL(k_cfg_sampler_masked<T>, dim3(i2i_grid(((n_img + 3) >> 2) * B)), dim3(I2I_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps2,
                     (float*)x0_hist, (const float*)params, (const float*)coeffs, rows, (const float*)x0_init, (const float*)mask, B, C, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

extern "C" {

int tf_image_from_u8_f16(void* out, const void* x, long long n, tfStream_t s) {
  TF_REQUIRE(out && x && n >= 0, "tf_image_from_u8_f16: bad arguments (n=%lld)", n);
  if (n == 0) return TF_OK;
  const bool vec = n % 4 == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)x & 3) == 0;
  const int grid = i2i_grid((n + 3) >> 2);
  if (vec)
    hipLaunchKernelGGL(k_image_from_u8<true>, dim3(grid), dim3(I2I_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)x, n);
  else
    hipLaunchKernelGGL(k_image_from_u8<false>, dim3(grid), dim3(I2I_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)x, n);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_means_to_latent_f32(void* x0, const void* means, int B, int H, int W, tfStream_t s) {
  TF_REQUIRE(x0 && means && B >= 0 && H >= 0 && W >= 0, "tf_means_to_latent_f32: bad arguments (B=%d H=%d W=%d)", B, H, W);
  TF_REQUIRE(((uintptr_t)means & 7) == 0, "tf_means_to_latent_f32: means must be 8-byte aligned (one 4-channel fp16 pixel)");
  const long long total = (long long)B * H * W;
  TF_REQUIRE((long long)H * W < (1LL << 31), "tf_means_to_latent_f32: %lld pixels per image", (long long)H * W);
  if (total == 0) return TF_OK;
  hipLaunchKernelGGL(k_means_to_latent, dim3(i2i_grid(total)), dim3(I2I_BLOCK), 0, tf_hs(s), (float*)x0, (const h4*)means, B, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_noise_to_level_f32(void* out, const void* x0, int images, long long per_image, float a, unsigned seed_lo, unsigned seed_hi, int image_offset,
                          tfStream_t s) {
  TF_REQUIRE(out && x0 && images >= 0 && per_image >= 0 && image_offset >= 0, "tf_noise_to_level_f32: bad arguments (images=%d per_image=%lld offset=%d)",
             images, per_image, image_offset);
  TF_REQUIRE(a > 0.0f && a <= 1.0f, "tf_noise_to_level_f32: the level a = %g must lie in (0, 1]", (double)a);
  TF_REQUIRE(per_image <= (1LL << 32), "tf_noise_to_level_f32: %lld elements per image exceed the 2^32 Philox counters of an image", per_image);
  TF_REQUIRE(out == x0 || (const char*)out + images * per_image * 4 <= (const char*)x0 || (const char*)x0 + images * per_image * 4 <= (const char*)out,
             "tf_noise_to_level_f32: out and x0 overlap without being the same array");
  if (images == 0 || per_image == 0) return TF_OK;
  hipLaunchKernelGGL(k_noise_to_level, dim3(i2i_grid(((per_image + 3) >> 2) * images)), dim3(I2I_BLOCK), 0, tf_hs(s), (float*)out, (const float*)x0,
                     per_image, images, a, seed_lo, seed_hi, (u32)image_offset);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_cfg_sampler_step_masked_f32(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, const void* x0_init,
                                   const void* mask, int B, int C, int H, int W, tfStream_t s) {
  return cfg_sampler_step_masked<half_t>("tf_cfg_sampler_step_masked_f32", latent, eps2, x0_hist, params, coeffs, rows, x0_init, mask, B, C, H, W, s);
}

int tf_cfg_sampler_step_masked_bf16(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, const void* x0_init,
                                    const void* mask, int B, int C, int H, int W, tfStream_t s) {
  return cfg_sampler_step_masked<bf16_t>("tf_cfg_sampler_step_masked_bf16", latent, eps2, x0_hist, params, coeffs, rows, x0_init, mask, B, C, H, W, s);
}

}  // extern "C"
