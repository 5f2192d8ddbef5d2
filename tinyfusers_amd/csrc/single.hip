// The guidance-free step of variants/sd.py's compile(..., cfg=False): ONE guidance group instead of the CFG pair of variants/sd.py:31 and
// :44.  LCM and LCM-LoRA sample at guidance 1, where e = e_u + 1 (e_c - e_u) = e_c and the unconditional half of every launch is computed
// and thrown away; here the step opens with the latent stacked once (tf_latent_stack1_*) and ends in the sampler update on the one branch
// (tf_sampler_step1_*).  Own translation unit: no existing kernel's code changes.
//
// Philox tags as in csrc/img2img.hip: 1 = the ancestral noise of schedule row `step` (k_sampler1 draws what k_cfg_sampler draws), 2 = the
// noise that puts the known region of an inpainting step on its trajectory (what k_cfg_sampler_masked draws).
#include "common.h"
#include "philox.h"
#include "../../include/tinyfusers_hip.h"

#define S1_BLOCK 256

static inline int s1_grid(long long nthreads) {
  long long g = (nthreads + S1_BLOCK - 1) / S1_BLOCK;
  if (g > 256 * 8) g = 256 * 8;   // grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// latent (B,C,HW) f32 [, cond (B,Cc,HW) f32] -> x (B, HW, C+Cc) 16-bit NHWC: group 0 of k_cfg_duplicate (Cc == 0, cond never read) or of
// k_cfg_concat with no dropped group, whose cast this is -- one thread per output element, consecutive threads on consecutive addresses.
template <typename T>
__global__ void __launch_bounds__(S1_BLOCK) k_latent_stack1(T* __restrict__ x, const float* __restrict__ lat, const float* __restrict__ cond, int B, int C, int Cc,
                                                            int HW) {
  const int Ct = C + Cc;
  const long long n = (long long)B * HW * Ct, gs = (long long)gridDim.x * S1_BLOCK;
  for (long long i = (long long)blockIdx.x * S1_BLOCK + threadIdx.x; i < n; i += gs) {
    const int c = (int)(i % Ct);
    const long long p = i / Ct;
    const int hw = (int)(p % HW), b = (int)(p / HW);
    x[i] = c >= C ? (T)cond[((long long)b * Cc + (c - C)) * HW + hw] : (T)lat[((long long)b * C + c) * HW + hw];
  }
}

// k_cfg_sampler (csrc/sampler.hip) without the CFG combine: e = eps (B, HW, C), one branch; from there its expressions in its order:
// x0 = (x - sqrt(1-a_t) e) / sqrt(a_t); x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z (tag 1); x0_prev <- x0.  MASKED: then the blend of
// k_cfg_sampler_masked (csrc/img2img.hip): x' <- m x' + (1 - m) (sqrt(a_s) x0_init + sqrt(1 - a_s) z2), a_s = params[2], z2 the tag-2 normal,
// always drawn.  x0_prev is read only when c_1 != 0, the tag-1 noise drawn only when c_n != 0; params[3] (guidance) is not read.
// One thread per Philox counter: 4 NCHW elements.
template <typename T, bool MASKED>
__global__ void __launch_bounds__(S1_BLOCK) k_sampler1(float* __restrict__ lat, const T* __restrict__ eps, float* __restrict__ x0h,
                                                       const float* __restrict__ params, const float* __restrict__ coeffs, int rows,
                                                       const float* __restrict__ x0i, const float* __restrict__ mask, int B, int C, int HW) {
  const u32* w = reinterpret_cast<const u32*>(params);
  const float a_t = params[1], a_s = params[2];
  u32 row = w[4];
  if (row >= (u32)rows) row = (u32)rows - 1;                     // memory safety only: the host entry writes a row of the schedule
  const u32 k0 = w[5], k1 = w[6], image0 = w[7];
  const float cx = coeffs[4 * row], c0 = coeffs[4 * row + 1], c1 = coeffs[4 * row + 2], cn = coeffs[4 * row + 3];
  const float s1 = sqrtf(1.0f - a_t), r = sqrtf(a_t);
  const float ra = sqrtf(a_s), rn = sqrtf(1.0f - a_s);
  const long long n_img = (long long)C * HW, nq = (n_img + 3) >> 2, total = nq * B, gs = (long long)gridDim.x * S1_BLOCK;
  for (long long t = (long long)blockIdx.x * S1_BLOCK + threadIdx.x; t < total; t += gs) {
    const int b = (int)(t / nq);
    const long long q = t - (long long)b * nq;
    float z[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f};
    if (cn != 0.f) normal4(k0, k1, (u32)q, image0 + (u32)b, row, 1u, z);
    if (MASKED) normal4(k0, k1, (u32)q, image0 + (u32)b, row, 2u, z2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * q + j;
      if (e >= n_img) break;
      const int c = (int)(e / HW), hw = (int)(e - (long long)c * HW);
      const long long i = (long long)b * n_img + e, je = ((long long)b * HW + hw) * C + c;
      const float ee = (float)eps[je];
      const float x = lat[i];
      const float x0 = (x - s1 * ee) / r;
      float xn = cx * x + c0 * x0;
      if (c1 != 0.f) xn += c1 * x0h[i];
      if (cn != 0.f) xn += cn * z[j];
      if (MASKED) {
        const float m = mask[(long long)b * HW + hw];
        const float kn = ra * x0i[i] + rn * z2[j];
        xn = m * xn + (1.0f - m) * kn;
      }
      lat[i] = xn;
      x0h[i] = x0;
    }
  }
}

template <typename T>
static int latent_stack1(const char* name, void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s) {
  TF_REQUIRE(x_out && latent && B > 0 && C > 0 && Cc >= 0 && H > 0 && W > 0, "%s: bad arguments (B=%d C=%d Cc=%d H=%d W=%d)", name, B, C, Cc, H, W);
  TF_REQUIRE((cond != nullptr) == (Cc > 0), "%s: cond is %s with Cc=%d (cond == NULL iff Cc == 0)", name, cond ? "set" : "NULL", Cc);
  TF_REQUIRE((long long)H * W < (1LL << 31) && (long long)C + Cc < (1LL << 16), "%s: %lld pixels of %lld channels", name, (long long)H * W, (long long)C + Cc);
  TF_REQUIRE(((uintptr_t)x_out & 1) == 0, "%s: x_out must be 2-byte aligned", name);
  const long long n = (long long)B * H * W * (C + Cc);
  hipLaunchKernelGGL(k_latent_stack1<T>, dim3(s1_grid(n)), dim3(S1_BLOCK), 0, tf_hs(s), (T*)x_out, (const float*)latent, (const float*)cond, B, C, Cc, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

template <typename T>
static int sampler_step1(const char* name, void* latent, const void* eps, void* x0_hist, const void* params, const void* coeffs, int rows, const void* x0_init,
                         const void* mask, int B, int C, int H, int W, tfStream_t s) {
  TF_REQUIRE(latent && eps && x0_hist && params && coeffs && rows >= 1 && B > 0 && C > 0 && H > 0 && W > 0, "%s: bad arguments (rows=%d B=%d C=%d H=%d W=%d)", name,
             rows, B, C, H, W);
  TF_REQUIRE((x0_init != nullptr) == (mask != nullptr), "%s: bad arguments (x0_init and mask go together: both set for the masked form, both NULL for the plain one)", name);
  const long long n_img = (long long)C * H * W;
  TF_REQUIRE(n_img <= (1LL << 32), "%s: %lld elements per image exceed the 2^32 Philox counters of an image", name, n_img);
  const dim3 grid(s1_grid(((n_img + 3) >> 2) * B));
  if (mask)
    hipLaunchKernelGGL((k_sampler1<T, true>), grid, dim3(S1_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps, (float*)x0_hist, (const float*)params,
                       (const float*)coeffs, rows, (const float*)x0_init, (const float*)mask, B, C, H * W);
  else
    hipLaunchKernelGGL((k_sampler1<T, false>), grid, dim3(S1_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps, (float*)x0_hist, (const float*)params,
                       (const float*)coeffs, rows, (const float*)nullptr, (const float*)nullptr, B, C, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

extern "C" {

int tf_latent_stack1_f16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s) {
  return latent_stack1<half_t>("tf_latent_stack1_f16", x_out, latent, cond, B, C, Cc, H, W, s);
}

int tf_latent_stack1_bf16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s) {
  return latent_stack1<bf16_t>("tf_latent_stack1_bf16", x_out, latent, cond, B, C, Cc, H, W, s);
}

int tf_sampler_step1_f32(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init, const void* mask,
                         int B, int C, int H, int W, tfStream_t s) {
  return sampler_step1<half_t>("tf_sampler_step1_f32", latent, eps, x0_hist, step_params, coeffs, rows, x0_init, mask, B, C, H, W, s);
}

int tf_sampler_step1_bf16(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init, const void* mask,
                          int B, int C, int H, int W, tfStream_t s) {
  return sampler_step1<bf16_t>("tf_sampler_step1_bf16", latent, eps, x0_hist, step_params, coeffs, rows, x0_init, mask, B, C, H, W, s);
}

}  // extern "C"
