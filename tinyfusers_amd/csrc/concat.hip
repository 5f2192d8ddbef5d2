// Concat-conditioned SD-1.x UNets on the sampler of csrc/sampler.hip: the inpainting checkpoint reads [latent(4) | mask(1) | latent of the
// masked image(4)], InstructPix2Pix reads [latent(4) | latent of the image to edit(4)] and combines three guidance branches.  The opening
// launch of the step (variants/sd.py:31 with the conditioning channels appended), the three-branch update, and the two edges of the VAE
// encoder that fill the conditioning buffer (vae/vae.py:12-15).  Own translation unit: no existing kernel's code changes.
//
// Philox tags as in csrc/img2img.hip: 1 = the ancestral noise of schedule row `step` (k_cfg3_sampler draws what k_cfg_sampler draws).
#include "common.h"
#include "philox.h"
#include "../../include/tinyfusers_hip.h"

#define CC_BLOCK 256

static inline int cc_grid(long long nthreads) {
  long long g = (nthreads + CC_BLOCK - 1) / CC_BLOCK;
  if (g > 256 * 8) g = 256 * 8;   // grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// latent (B,C,HW) f32, cond (B,Cc,HW) f32 -> x (G*B, HW, C+Cc) 16-bit NHWC: every group the same [latent | cond] pixels, the cond channels +0
// in the groups whose bit of `drop` is set (bits at or above G name no group and are ignored).  A pixel is 2 (C+Cc) bytes (18 for the
// inpainting model), so nothing above the element's own 2-byte alignment holds for a pixel start: one thread per output element of a
// group, consecutive threads on consecutive addresses (the store pattern of k_cfg_duplicate, whose cast this is: the latent channels are
// its output bit for bit).
template <typename T>
__global__ void __launch_bounds__(CC_BLOCK) k_cfg_concat(T* __restrict__ x, const float* __restrict__ lat, const float* __restrict__ cond, int B, int C, int Cc,
                                                         int HW, int G, unsigned drop) {
  const int Ct = C + Cc;
  const long long n = (long long)B * HW * Ct, gs = (long long)gridDim.x * CC_BLOCK;
  for (long long i = (long long)blockIdx.x * CC_BLOCK + threadIdx.x; i < n; i += gs) {
    const int c = (int)(i % Ct);
    const long long p = i / Ct;
    const int hw = (int)(p % HW), b = (int)(p / HW);
    const bool is_cond = c >= C;
    const T v = is_cond ? (T)cond[((long long)b * Cc + (c - C)) * HW + hw] : (T)lat[((long long)b * C + c) * HW + hw];
    const T zero = (T)0.0f;
    for (int g = 0; g < G; ++g) x[(long long)g * n + i] = (is_cond && ((drop >> g) & 1u)) ? zero : v;
  }
}

// k_cfg_sampler (csrc/sampler.hip) with three guidance branches, eps3 = [e0 ; e1 ; e2] (3B, HW, C):
// e = e0 + g_T (e2 - e1) + g_I (e1 - e0), g_T = params[3], g_I = edit[0]; from there its expressions in its order:
// x0 = (x - sqrt(1-a_t) e) / sqrt(a_t); x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z (tag 1); x0_prev <- x0.
template <typename T>
__global__ void __launch_bounds__(CC_BLOCK) k_cfg3_sampler(float* __restrict__ lat, const T* __restrict__ eps3, float* __restrict__ x0h,
                                                           const float* __restrict__ params, const float* __restrict__ coeffs, int rows,
                                                           const float* __restrict__ edit, int B, int C, int HW) {
  const u32* w = reinterpret_cast<const u32*>(params);
  const float a_t = params[1], gt = params[3], gi = edit[0];
  u32 row = w[4];
  if (row >= (u32)rows) row = (u32)rows - 1;                     // memory safety only: the host entry writes a row of the schedule
  const u32 k0 = w[5], k1 = w[6], image0 = w[7];
  const float cx = coeffs[4 * row], c0 = coeffs[4 * row + 1], c1 = coeffs[4 * row + 2], cn = coeffs[4 * row + 3];
  const float s1 = sqrtf(1.0f - a_t), r = sqrtf(a_t);
  const long long n_img = (long long)C * HW, n = n_img * B, nq = (n_img + 3) >> 2, total = nq * B, gs = (long long)gridDim.x * CC_BLOCK;
  for (long long t = (long long)blockIdx.x * CC_BLOCK + threadIdx.x; t < total; t += gs) {
    const int b = (int)(t / nq);
    const long long q = t - (long long)b * nq;
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (cn != 0.f) normal4(k0, k1, (u32)q, image0 + (u32)b, row, 1u, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * q + j;
      if (e >= n_img) break;
      const int c = (int)(e / HW), hw = (int)(e - (long long)c * HW);
      const long long i = (long long)b * n_img + e, je = ((long long)b * HW + hw) * C + c;
      const float e0 = (float)eps3[je], e1 = (float)eps3[n + je], e2 = (float)eps3[2 * n + je];
      const float ee = e0 + gt * (e2 - e1) + gi * (e1 - e0);
      const float x = lat[i];
      const float x0 = (x - s1 * ee) / r;
      float xn = cx * x + c0 * x0;
      if (c1 != 0.f) xn += c1 * x0h[i];
      if (cn != 0.f) xn += cn * z[j];
      lat[i] = xn;
      x0h[i] = x0;
    }
  }
}

// u8_to_unit of csrc/img2img.hip restated: (2u - 255) / 255 = u / 127.5 - 1, one correctly rounded fp32 division, then fp16
__device__ __forceinline__ half_t cc_u8_to_unit(unsigned u) { return (half_t)((float)(2 * (int)u - 255) / 255.0f); }

// image (P, 3) uint8, mask (P) uint8 -> out (P, 3) fp16 = u / 127.5 - 1 where the pixel's mask byte is 0, +0 where it is not (the masked
// image of the inpainting model: the repainted region is grey, 0 in [-1, 1]).  One thread per element
__global__ void __launch_bounds__(CC_BLOCK) k_image_from_u8_masked(half_t* __restrict__ out, const unsigned char* __restrict__ in,
                                                                   const unsigned char* __restrict__ mask, long long n) {
  const long long gs = (long long)gridDim.x * CC_BLOCK;
  for (long long i = (long long)blockIdx.x * CC_BLOCK + threadIdx.x; i < n; i += gs) out[i] = mask[i / 3] ? (half_t)0.0f : cc_u8_to_unit(in[i]);
}

// k_means_to_latent (csrc/img2img.hip) with the scale an argument and the 4 channels written at [c_off, c_off + 4) of a (B, Ct, HW) buffer
__global__ void __launch_bounds__(CC_BLOCK) k_means_to_cond(float* __restrict__ cond, const h4* __restrict__ means, int B, int HW, float scale, int c_off, int Ct) {
  const long long total = (long long)B * HW, gs = (long long)gridDim.x * CC_BLOCK;
  for (long long t = (long long)blockIdx.x * CC_BLOCK + threadIdx.x; t < total; t += gs) {
    const int b = (int)(t / HW), hw = (int)(t - (long long)b * HW);
    const h4 m = means[t];
    float* o = cond + ((long long)b * Ct + c_off) * HW + hw;
    o[0] = scale * (float)m.x;
    o[HW] = scale * (float)m.y;
    o[2 * (long long)HW] = scale * (float)m.z;
    o[3 * (long long)HW] = scale * (float)m.w;
  }
}

template <typename T>
static int cfg_concat(const char* name, void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits,
                      tfStream_t s) {
  TF_REQUIRE(x_out && latent && cond && B > 0 && C > 0 && Cc > 0 && H > 0 && W > 0, "%s: bad arguments (B=%d C=%d Cc=%d H=%d W=%d)", name, B, C, Cc, H, W);
  TF_REQUIRE(groups == 2 || groups == 3, "%s: groups=%d (2 or 3)", name, groups);
  TF_REQUIRE((long long)H * W < (1LL << 31) && (long long)C + Cc < (1LL << 16), "%s: %lld pixels of %lld channels", name, (long long)H * W, (long long)C + Cc);
  TF_REQUIRE(((uintptr_t)x_out & 1) == 0, "%s: x_out must be 2-byte aligned", name);
  const long long n = (long long)B * H * W * (C + Cc);
  hipLaunchKernelGGL(k_cfg_concat<T>, dim3(cc_grid(n)), dim3(CC_BLOCK), 0, tf_hs(s), (T*)x_out, (const float*)latent, (const float*)cond, B, C, Cc, H * W, groups,
                     drop_bits);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

template <typename T>
static int cfg3_sampler_step(const char* name, void* latent, const void* eps3, void* x0_hist, const void* params, const void* coeffs, int rows, const void* edit,
                             int B, int C, int H, int W, tfStream_t s) {
  TF_REQUIRE(latent && eps3 && x0_hist && params && coeffs && edit && rows >= 1 && B > 0 && C > 0 && H > 0 && W > 0,
             "%s: bad arguments (rows=%d B=%d C=%d H=%d W=%d)", name, rows, B, C, H, W);
  const long long n_img = (long long)C * H * W;
  TF_REQUIRE(n_img <= (1LL << 32), "%s: %lld elements per image exceed the 2^32 Philox counters of an image", name, n_img);
  hipLaunchKernelGGL(k_cfg3_sampler<T>, dim3(cc_grid(((n_img + 3) >> 2) * B)), dim3(CC_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps3, (float*)x0_hist,
                     (const float*)params, (const float*)coeffs, rows, (const float*)edit, B, C, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

extern "C" {

int tf_cfg_concat_f16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s) {
  return cfg_concat<half_t>("tf_cfg_concat_f16", x_out, latent, cond, B, C, Cc, H, W, groups, drop_bits, s);
}

int tf_cfg_concat_bf16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s) {
  return cfg_concat<bf16_t>("tf_cfg_concat_bf16", x_out, latent, cond, B, C, Cc, H, W, groups, drop_bits, s);
}

int tf_cfg3_sampler_step_f32(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                             int B, int C, int H, int W, tfStream_t s) {
  return cfg3_sampler_step<half_t>("tf_cfg3_sampler_step_f32", latent, eps3, x0_hist, step_params, coeffs, rows, edit_params, B, C, H, W, s);
}

int tf_cfg3_sampler_step_bf16(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                              int B, int C, int H, int W, tfStream_t s) {
  return cfg3_sampler_step<bf16_t>("tf_cfg3_sampler_step_bf16", latent, eps3, x0_hist, step_params, coeffs, rows, edit_params, B, C, H, W, s);
}

int tf_image_from_u8_masked_f16(void* out, const void* image_u8, const void* mask_u8, int B, int H, int W, tfStream_t s) {
  TF_REQUIRE(out && image_u8 && mask_u8 && B >= 0 && H >= 0 && W >= 0, "tf_image_from_u8_masked_f16: bad arguments (B=%d H=%d W=%d)", B, H, W);
  TF_REQUIRE(((uintptr_t)out & 1) == 0, "tf_image_from_u8_masked_f16: out must be 2-byte aligned");
  const long long n = 3LL * B * H * W;
  if (n == 0) return TF_OK;
  hipLaunchKernelGGL(k_image_from_u8_masked, dim3(cc_grid(n)), dim3(CC_BLOCK), 0, tf_hs(s), (half_t*)out, (const unsigned char*)image_u8,
                     (const unsigned char*)mask_u8, n);
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
  hipLaunchKernelGGL(k_means_to_cond, dim3(cc_grid(total)), dim3(CC_BLOCK), 0, tf_hs(s), (float*)cond, (const h4*)means, B, H * W, scale, c_off, c_total);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

}  // extern "C"
