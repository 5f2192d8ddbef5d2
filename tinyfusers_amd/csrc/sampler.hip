// Samplers beyond the reference's sigma = 0 DDIM update (variants/sd.py:14-25): the device-side normal generator and the fused
// CFG + sampler update of tinyfusers_amd/variants/samplers.py.  Own translation unit: no existing kernel's code changes.
//
// Noise is Philox4x32-10 (Salmon et al. 2011, Random123), key = the 64-bit seed, counter = (q, global image index, step, tag); the q-th
// counter of an image gives its NCHW elements 4q .. 4q+3 through two Box-Muller pairs.  An image's noise therefore depends on the seed, its
// global index, the step and the tag only -- not on the batch size, the rank that owns it, or whether it is drawn by tf_randn_f32 or inline
// by the sampler update.  Tags: 0 the initial latent, 1 the ancestral noise of a step (step = schedule index); the generator is in philox.h.
#include "common.h"
#include "philox.h"
#include "../../include/tinyfusers_hip.h"

#define SM_BLOCK 256
enum { TF_SAMPLER_PARAM_WORDS = 8 };   // [0] t [1] a_t [2] a_prev [3] guidance (fp32) | [4] row [5] seed lo [6] seed hi [7] image offset (u32)

static inline int sm_grid(long long nthreads) {
  long long g = (nthreads + SM_BLOCK - 1) / SM_BLOCK;
  if (g > 256 * 8) g = 256 * 8;   // grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// out: `images` fp32 NCHW images of n_img elements each; image k is global image image0 + k
__global__ void __launch_bounds__(SM_BLOCK) k_randn(float* __restrict__ out, long long n_img, int images, u32 k0, u32 k1, u32 image0, u32 step, u32 tag) {
  const long long nq = (n_img + 3) >> 2, total = nq * images, gs = (long long)gridDim.x * SM_BLOCK;
  for (long long t = (long long)blockIdx.x * SM_BLOCK + threadIdx.x; t < total; t += gs) {
    const int k = (int)(t / nq);
    const long long q = t - (long long)k * nq;
    float z[4];
    normal4(k0, k1, (u32)q, image0 + (u32)k, step, tag, z);
    float* o = out + (long long)k * n_img + 4 * q;
    const long long left = n_img - 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < left) o[j] = z[j];
  }
}

// the step scalars of k_set_params_copy (elementwise.hip) plus the sampler words, in the launch that already runs ahead of every replay
__global__ void __launch_bounds__(256) k_set_sampler_params(float* p, float t, float a_t, float a_prev, float g, u32 row, u32 seed_lo, u32 seed_hi, u32 image0,
                                                            uint4* __restrict__ dst, const uint4* __restrict__ src, long long n16) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    p[0] = t; p[1] = a_t; p[2] = a_prev; p[3] = g;
    u32* w = reinterpret_cast<u32*>(p);
    w[4] = row; w[5] = seed_lo; w[6] = seed_hi; w[7] = image0;
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

// e = e_u + g (e_c - e_u); x0 = (x - sqrt(1-a_t) e) / sqrt(a_t); x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z; x0_prev <- x0.
// [c_x, c_0, c_1, c_n] = coeffs[row], row = the schedule index the parameter launch wrote.  x0_prev is read only when c_1 != 0 (a fresh
// history never reaches the first step) and the noise is drawn only when c_n != 0.  One thread per Philox counter: 4 NCHW elements.
template <typename T>
__global__ void __launch_bounds__(SM_BLOCK) k_cfg_sampler(float* __restrict__ lat, const T* __restrict__ eps2, float* __restrict__ x0h,
                                                          const float* __restrict__ params, const float* __restrict__ coeffs, int rows, int B, int C, int HW) {
  const u32* w = reinterpret_cast<const u32*>(params);
  const float a_t = params[1], g = params[3];
  u32 row = w[4];
  if (row >= (u32)rows) row = (u32)rows - 1;                     // memory safety only: the host entry writes a row of the schedule
  const u32 k0 = w[5], k1 = w[6], image0 = w[7];
  const float cx = coeffs[4 * row], c0 = coeffs[4 * row + 1], c1 = coeffs[4 * row + 2], cn = coeffs[4 * row + 3];
  const float s1 = sqrtf(1.0f - a_t), r = sqrtf(a_t);
  const long long n_img = (long long)C * HW, n = n_img * B, nq = (n_img + 3) >> 2, total = nq * B, gs = (long long)gridDim.x * SM_BLOCK;
  for (long long t = (long long)blockIdx.x * SM_BLOCK + threadIdx.x; t < total; t += gs) {
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
      const float eu = (float)eps2[je], ec = (float)eps2[n + je];
      const float ee = eu + g * (ec - eu);
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

template <typename T>
static int cfg_sampler_step(const char* name, void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, int B, int C, int H, int W,
                            tfStream_t s) {
  TF_REQUIRE(latent && eps2 && x0_hist && params && coeffs && rows >= 1 && B > 0 && C > 0 && H > 0 && W > 0, "%s: bad arguments (rows=%d B=%d C=%d H=%d W=%d)", name, rows, B, C, H, W);
  const long long n_img = (long long)C * H * W;
  TF_REQUIRE(n_img <= (1LL << 32), "%s: %lld elements per image exceed the 2^32 Philox counters of an image", name, n_img);
  hipLaunchKernelGGL(k_cfg_sampler<T>, dim3(sm_grid(((n_img + 3) >> 2) * B)), dim3(SM_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps2, (float*)x0_hist,
                     (const float*)params, (const float*)coeffs, rows, B, C, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

extern "C" {

int tf_randn_f32(void* out, int images, long long per_image, unsigned seed_lo, unsigned seed_hi, int image_offset, int step, int tag, tfStream_t s) {
  TF_REQUIRE(out && images >= 0 && per_image >= 0 && image_offset >= 0 && step >= 0 && tag >= 0, "tf_randn_f32: bad arguments (images=%d per_image=%lld offset=%d step=%d tag=%d)",
             images, per_image, image_offset, step, tag);
  TF_REQUIRE(per_image <= (1LL << 32), "tf_randn_f32: %lld elements per image exceed the 2^32 Philox counters of an image", per_image);
  if (images == 0 || per_image == 0) return TF_OK;
  hipLaunchKernelGGL(k_randn, dim3(sm_grid(((per_image + 3) >> 2) * images)), dim3(SM_BLOCK), 0, tf_hs(s), (float*)out, per_image, images, seed_lo, seed_hi,
                     (u32)image_offset, (u32)step, (u32)tag);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_set_sampler_params(void* step_params, float timestep, float a_t, float a_prev, float guidance, int row, unsigned seed_lo, unsigned seed_hi, int image_offset,
                          void* dst, const void* src, long long nbytes, tfStream_t s) {
  TF_REQUIRE(step_params && row >= 0 && image_offset >= 0 && nbytes >= 0 && nbytes % 16 == 0 && (nbytes == 0 || (dst && src)),
             "tf_set_sampler_params: bad arguments (row=%d image_offset=%d nbytes=%lld, a multiple of 16 with both pointers set)", row, image_offset, nbytes);
  TF_REQUIRE((((uintptr_t)dst | (uintptr_t)src) & 15) == 0, "tf_set_sampler_params: dst and src must be 16-byte aligned");
  const long long n16 = nbytes / 16;
  int grid = (int)((n16 + 255) / 256);
  if (grid < 1) grid = 1;
  if (grid > 64) grid = 64;
  hipLaunchKernelGGL(k_set_sampler_params, dim3(grid), dim3(256), 0, tf_hs(s), (float*)step_params, timestep, a_t, a_prev, guidance, (u32)row, seed_lo, seed_hi,
                     (u32)image_offset, (uint4*)dst, (const uint4*)src, n16);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

int tf_cfg_sampler_step_f32(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, int B, int C, int H, int W, tfStream_t s) {
  return cfg_sampler_step<half_t>("tf_cfg_sampler_step_f32", latent, eps2, x0_hist, params, coeffs, rows, B, C, H, W, s);
}

int tf_cfg_sampler_step_bf16(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, int B, int C, int H, int W, tfStream_t s) {
  return cfg_sampler_step<bf16_t>("tf_cfg_sampler_step_bf16", latent, eps2, x0_hist, params, coeffs, rows, B, C, H, W, s);
}

}  // extern "C"
