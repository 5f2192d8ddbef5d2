// The sampler side of the captured step for every mode of tinyfusers_amd/variants/sd.py (the CFG pair, the inpainting blend, the concat
// checkpoints' two or three guidance groups, the guidance-free single branch): the device-side normal generator, the parameter launch, the
// step's HEAD (the latent stacked for the UNet: variants/sd.py:31) and its TAIL (guidance combine + sampler update, generalising
// variants/sd.py:14-25 and :27-46; the coefficient rows are tinyfusers_amd/variants/samplers.py's).  Each kernel exists once; the C entries
// differ in what their parameters mean and in which argument sets they refuse.
//
// Noise is Philox4x32-10 (Salmon et al. 2011, Random123; the generator is in philox.h), key = the 64-bit seed, counter = (q, global image
// index, step, tag); the q-th counter of an image gives its NCHW elements 4q .. 4q+3 through two Box-Muller pairs.  An image's noise
// therefore depends on the seed, its global index, the step and the tag only -- not on the batch size, the rank that owns it, or whether it
// is drawn by tf_randn_f32 or inline by the sampler update.  Tags:
//   0  the initial latent: tf_randn_f32 and tf_noise_to_level_f32 (step 0) draw the same z, so an img2img image and a text-to-image image of
//      one seed share their noise
//   1  the ancestral noise of schedule row `step` (k_sampler_step, every form)
//   2  the noise that puts the known region of an inpainting step on its trajectory, step = the schedule row (k_sampler_step, MASKED)
#include "common.h"
#include "philox.h"
#include "../../include/tinyfusers_hip.h"

enum { TF_SAMPLER_PARAM_WORDS = 8 };   // [0] t [1] a_t [2] a_prev [3] guidance (fp32) | [4] row [5] seed lo [6] seed hi [7] image offset (u32)

// out: `images` fp32 NCHW images of n_img elements each; image k is global image image0 + k
__global__ void __launch_bounds__(EW_BLOCK) k_randn(float* __restrict__ out, long long n_img, int images, u32 k0, u32 k1, u32 image0, u32 step, u32 tag) {
  const long long nq = (n_img + 3) >> 2, total = nq * images, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; t < total; t += gs) {
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

// out = sqrt(a) x0 + sqrt(1 - a) z, z the tag-0 normal of global image image0 + k at step 0.  out may alias x0 (each element is read, then
// written, by the same thread).  One thread per Philox counter: 4 NCHW elements
__global__ void __launch_bounds__(EW_BLOCK) k_noise_to_level(float* out, const float* x0, long long n_img, int images, float a, u32 k0, u32 k1, u32 image0) {
  const float sa = sqrtf(a), sn = sqrtf(1.0f - a);
  const long long nq = (n_img + 3) >> 2, total = nq * images, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; t < total; t += gs) {
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

// The head: latent (B,C,HW) f32 [, cond (B,Cc,HW) f32] -> x (G*B, HW, C+Cc) 16-bit NHWC: every group the same [latent | cond] pixels, the
// cond channels +0 in the groups whose bit of `drop` is set (bits at or above G name no group and are ignored).  Cc == 0: cond is never
// read.  A pixel is 2 (C+Cc) bytes (18 for the inpainting model), so nothing above the element's own 2-byte alignment holds for a pixel
// start: one thread per output element of a group, consecutive threads on consecutive addresses.  G is compile-time: the G stores unroll, as
// the CFG pair's two always did (the launch of the benchmark path), in 19 VGPRs where a runtime loop takes 23.
template <typename T, int G>
__global__ void __launch_bounds__(EW_BLOCK) k_latent_stack(T* __restrict__ x, const float* __restrict__ lat, const float* __restrict__ cond, int B, int C, int Cc,
                                                           int HW, unsigned drop) {
  const int Ct = C + Cc;
  const long long n = (long long)B * HW * Ct, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long i = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; i < n; i += gs) {
    const int c = (int)(i % Ct);
    const long long p = i / Ct;
    const int hw = (int)(p % HW), b = (int)(p / HW);
    const bool is_cond = c >= C;
    const T v = is_cond ? (T)cond[((long long)b * Cc + (c - C)) * HW + hw] : (T)lat[((long long)b * C + c) * HW + hw];
    const T zero = (T)0.0f;
    for (int g = 0; g < G; ++g) x[(long long)g * n + i] = (is_cond && ((drop >> g) & 1u)) ? zero : v;
  }
}

// The tail.  eps = G guidance groups of (B, HW, C) 16-bit NHWC, combined into e:
//   G = 1  e = eps                                  (params[3], the guidance, is not read)
//   G = 2  e = e_u + g (e_c - e_u)                  g = params[3]
//   G = 3  e = e0 + g_T (e2 - e1) + g_I (e1 - e0)   g_T = params[3], g_I = edit[0]  (an edit model's [x|0, unc ; x|c, unc ; x|c, ctx]; perturbed-
//          attention guidance's [uncond ; perturbed ; cond] at g_I = g, g_T = g + s: e_u + g (e_c - e_u) + s (e_c - e_p))
// then x0 = (x - sqrt(1-a_t) e) / sqrt(a_t); x' = c_x x + c_0 x0 + c_1 x0_prev + c_n z (tag 1); x0_prev <- x0.  [c_x, c_0, c_1, c_n] =
// coeffs[row], row = the schedule index the parameter launch wrote.  x0_prev is read only when c_1 != 0 (a fresh history never reaches the
// first step) and the tag-1 noise is drawn only when c_n != 0.  MASKED: then the inpainting blend
// x' <- m x' + (1 - m) (sqrt(a_s) x0_init + sqrt(1 - a_s) z2), a_s = params[2] (the a_prev of tf_set_sampler_params), z2 the tag-2 normal at
// step = row, always drawn.  m = 1 leaves x' as it is (1 x' + 0); m = 0 at the last step (a_s = 1) gives x0_init exactly.  mask (B, 1, H, W)
// fp32.  G and MASKED are compile-time, and every form keeps these expressions in this order: -ffp-contract=fast contracts by expression
// shape, and the sampled trajectories are compared bit for bit.  One thread per Philox counter: 4 NCHW elements.
template <typename T, int G, bool MASKED>
__global__ void __launch_bounds__(EW_BLOCK) k_sampler_step(float* __restrict__ lat, const T* __restrict__ eps, float* __restrict__ x0h,
                                                           const float* __restrict__ params, const float* __restrict__ coeffs, int rows,
                                                           const float* __restrict__ edit, const float* __restrict__ x0i, const float* __restrict__ mask,
                                                           int B, int C, int HW) {
  const u32* w = reinterpret_cast<const u32*>(params);
  const float a_t = params[1], a_s = params[2];
  const float g = G >= 2 ? params[3] : 0.f, gi = G == 3 ? edit[0] : 0.f;
  u32 row = w[4];
  if (row >= (u32)rows) row = (u32)rows - 1;                     // memory safety only: the host entry writes a row of the schedule
  const u32 k0 = w[5], k1 = w[6], image0 = w[7];
  const float cx = coeffs[4 * row], c0 = coeffs[4 * row + 1], c1 = coeffs[4 * row + 2], cn = coeffs[4 * row + 3];
  const float s1 = sqrtf(1.0f - a_t), r = sqrtf(a_t);
  const float ra = sqrtf(a_s), rn = sqrtf(1.0f - a_s);
  const long long n_img = (long long)C * HW, n = n_img * B, nq = (n_img + 3) >> 2, total = nq * B, gs = (long long)gridDim.x * EW_BLOCK;
  for (long long t = (long long)blockIdx.x * EW_BLOCK + threadIdx.x; t < total; t += gs) {
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
      float ee;
      if (G == 1) {
        ee = (float)eps[je];
      } else if (G == 2) {
        const float eu = (float)eps[je], ec = (float)eps[n + je];
        ee = eu + g * (ec - eu);
      } else {
        const float e0 = (float)eps[je], e1 = (float)eps[n + je], e2 = (float)eps[2 * n + je];
        ee = e0 + g * (e2 - e1) + gi * (e1 - e0);
      }
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

// ---- the tail with v-prediction and CFG rescale: k_sampler_step_rescale<T, G>, the kernel behind every tf_sampler_tail_* call that sets bit 0 or
// bit 2.  The masked blend, the parameterisation and the rescale are RUN-TIME flags (wave-uniform branches), not template parameters: the library's
// kernel census is capped (tests/test_abi.py) and 2 x 3 instances fit where 2 x 3 x 2 x 2 do not.  Its arithmetic is therefore STATED, operation by
// operation (contraction off in the kernel body, fmaf where k_sampler_step's instances fuse), as the twelve k_sampler_step instances compile theirs --
// read off their assembly, the same in all twelve: e = fma(g, e_c - e_u, e_u) (three groups: fma(g_I, e1 - e0, fma(g_T, e2 - e1, e0))),
// x0 = fma(-s1, e, x) / r, x' = (c_x x) + (c_0 x0) unfused, then fma(c_1, x0_prev, .), fma(c_n, z, .); the known region fma(ra, x0_init, rn z2) and the
// blend (m x') + ((1 - m) known) unfused -- so that the eps forms at phi = 0 return k_sampler_step's bits.
// v-prediction (Salimans & Ho 2022; the SD-2.x 768-v checkpoints): e is v and the x0 line alone changes, x0 = fma(-s1, v, r x).
// ---- CFG rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed" 3.4; diffusers'
// rescale_noise_cfg): the combined output e is pulled back to the standard deviation of the text group e_t -- the LAST guidance group --
// per image, over its C H W elements:  f = std(e_t) / std(e) (1 where std(e) == 0),  e' = phi (e f) + (1 - phi) e,  and k_sampler_step's
// update runs on e'.  phi: one fp32 word on the device.
// ONE block per image, three sweeps over the image's groups (after the first they come out of L2): the sums of (e - p_e), (e_t - p_t) around
// the pivots p = the image's element 0 (a constant image sums zeros: its mean is exact and its f is 1), then the sums of the squared
// deviations from those means (two passes: a mean of 8 sigma costs nothing), then the update.  Every sum has ONE order, whatever the launch:
// thread t adds the elements of the 8-element chunks t, t + 1024, ... of the image's NHWC memory in element order, a wave adds its lanes by
// the xor butterfly (wave_sum), and every thread adds the 16 wave partials from LDS in wave order.  No atomics; image k's result depends on
// image k alone -- not on B, not on what else the launch holds, and not on eps' alignment (the 16-byte loads of the chunked sweeps and the
// element loads they fall back to feed the same additions).
enum { RS_BLOCK = 1024, RS_WAVES = RS_BLOCK / 64 };

// e of the header comment of k_sampler_step from the groups' elements at one index, in the operations its instances compile to
template <int G>
__device__ __forceinline__ float tail_combine(float e0, float e1, float e2, float g, float gi) {
  if (G == 1) return e0;
  if (G == 2) return fmaf(g, e1 - e0, e0);
  return fmaf(gi, e1 - e0, fmaf(g, e2 - e1, e0));
}

// up to 8 consecutive 16-bit elements at p as floats (those at or behind `left` are not read and come back 0); vec: one 16-byte load
template <typename T>
__device__ __forceinline__ void load8(const T* __restrict__ p, long long left, bool vec, float (&out)[8]) {
  if (vec) {
    struct alignas(16) Raw { T v[8]; };
    const Raw raw = *reinterpret_cast<const Raw*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (float)raw.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = j < left ? (float)p[j] : 0.f;
  }
}

// (a, b) summed over the block in the fixed order above; every thread gets the two sums.  sh: 2 RS_WAVES floats nothing else uses
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sh) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) {
    sh[2 * (threadIdx.x >> 6)] = a;
    sh[2 * (threadIdx.x >> 6) + 1] = b;
  }
  __syncthreads();
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int i = 0; i < RS_WAVES; ++i) {
    sa += sh[2 * i];
    sb += sh[2 * i + 1];
  }
  a = sa;
  b = sb;
}

enum { TAIL_VPRED = 1u, TAIL_MASKED = 2u, TAIL_RESCALE = 4u };          // tf_sampler_tail_*'s flags

// flags & TAIL_RESCALE: the grid is B blocks, block b is image b.  Otherwise: any grid, the threads stride over every image's Philox counters as
// k_sampler_step's do, and `rescale` is not read.
template <typename T, int G>
__global__ void __launch_bounds__(RS_BLOCK) k_sampler_step_rescale(float* __restrict__ lat, const T* __restrict__ eps, float* __restrict__ x0h,
                                                                   const float* __restrict__ params, const float* __restrict__ coeffs, int rows,
                                                                   const float* __restrict__ edit, const float* __restrict__ x0i,
                                                                   const float* __restrict__ mask, const float* __restrict__ rescale, int B, int C, int HW,
                                                                   unsigned flags) {
#pragma clang fp contract(off)
  __shared__ float sh[2][2 * RS_WAVES];
  const bool vpred = flags & TAIL_VPRED, masked = flags & TAIL_MASKED, resc = (flags & TAIL_RESCALE) && G >= 2;
  const u32* w = reinterpret_cast<const u32*>(params);
  const float a_t = params[1], a_s = params[2];
  const float g = G >= 2 ? params[3] : 0.f, gi = G == 3 ? edit[0] : 0.f;
  u32 row = w[4];
  if (row >= (u32)rows) row = (u32)rows - 1;                     // memory safety only: the host entry writes a row of the schedule
  const u32 k0 = w[5], k1 = w[6], image0 = w[7];
  const float cx = coeffs[4 * row], c0 = coeffs[4 * row + 1], c1 = coeffs[4 * row + 2], cn = coeffs[4 * row + 3];
  const float s1 = sqrtf(1.0f - a_t), r = sqrtf(a_t);
  const float ra = sqrtf(a_s), rn = sqrtf(1.0f - a_s);
  const long long n_img = (long long)C * HW, n = n_img * B, nq = (n_img + 3) >> 2, nchunk = (n_img + 7) >> 3;
  float phi = 0.f, f = 1.0f;
  if (resc) {
    phi = rescale[0];
    const T* g0 = eps + (long long)blockIdx.x * n_img;           // this image in group 0; group k is n elements further
    const bool vec = (n_img & 7) == 0 && ((uintptr_t)eps & 15) == 0;
    // sweep 1: the means, around the pivots
    const float pt = (float)g0[(G - 1) * n];
    const float pe = tail_combine<G>((float)g0[0], (float)g0[G >= 2 ? n : 0], G == 3 ? (float)g0[2 * n] : 0.f, g, gi);
    float se = 0.f, st = 0.f;
    for (long long ch = threadIdx.x; ch < nchunk; ch += RS_BLOCK) {
      const long long left = n_img - 8 * ch;
      float v0[8], v1[8], v2[8];
      load8(g0 + 8 * ch, left, vec, v0);
      load8(g0 + (G >= 2 ? n : 0) + 8 * ch, left, vec, v1);
      if (G == 3) load8(g0 + 2 * n + 8 * ch, left, vec, v2);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < left) {
          se += tail_combine<G>(v0[j], v1[j], G == 3 ? v2[j] : 0.f, g, gi) - pe;
          st += (G == 3 ? v2[j] : v1[j]) - pt;
        }
    }
    block_sum2(se, st, sh[0]);
    const float me = pe + se / (float)n_img, mt = pt + st / (float)n_img;
    // sweep 2: the squared deviations
    float qe = 0.f, qt = 0.f;
    for (long long ch = threadIdx.x; ch < nchunk; ch += RS_BLOCK) {
      const long long left = n_img - 8 * ch;
      float v0[8], v1[8], v2[8];
      load8(g0 + 8 * ch, left, vec, v0);
      load8(g0 + (G >= 2 ? n : 0) + 8 * ch, left, vec, v1);
      if (G == 3) load8(g0 + 2 * n + 8 * ch, left, vec, v2);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < left) {
          const float de = tail_combine<G>(v0[j], v1[j], G == 3 ? v2[j] : 0.f, g, gi) - me;
          const float dt = (G == 3 ? v2[j] : v1[j]) - mt;
          qe = fmaf(de, de, qe);
          qt = fmaf(dt, dt, qt);
        }
    }
    block_sum2(qe, qt, sh[1]);
    f = qe > 0.f ? sqrtf(qt / qe) : 1.0f;                        // std(e_t) / std(e): the 1 / (n - 1) of both cancels
  }
  // the update: k_sampler_step's loop over Philox counters -- this block's image (rescale), or every image's across the grid
  const long long first = resc ? (long long)threadIdx.x : (long long)blockIdx.x * RS_BLOCK + threadIdx.x;
  const long long stride = resc ? (long long)RS_BLOCK : (long long)gridDim.x * RS_BLOCK, total = resc ? nq : nq * B;
  for (long long t = first; t < total; t += stride) {
    const int b = resc ? (int)blockIdx.x : (int)(t / nq);
    const long long q = resc ? t : t - (long long)b * nq;
    float z[4] = {0.f, 0.f, 0.f, 0.f}, z2[4] = {0.f, 0.f, 0.f, 0.f};
    if (cn != 0.f) normal4(k0, k1, (u32)q, image0 + (u32)b, row, 1u, z);
    if (masked) normal4(k0, k1, (u32)q, image0 + (u32)b, row, 2u, z2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long e = 4 * q + j;
      if (e >= n_img) break;
      const int c = (int)(e / HW), hw = (int)(e - (long long)c * HW);
      const long long i = (long long)b * n_img + e, je = ((long long)b * HW + hw) * C + c;
      float ee = tail_combine<G>((float)eps[je], G >= 2 ? (float)eps[n + je] : 0.f, G == 3 ? (float)eps[2 * n + je] : 0.f, g, gi);
      if (resc) {
        const float es = ee * f;
        ee = phi * es + (1.0f - phi) * ee;                       // (two products and a sum: exact at phi = 0 and at phi = 1)
      }
      const float x = lat[i];
      const float x0 = vpred ? fmaf(-s1, ee, r * x) : fmaf(-s1, ee, x) / r;
      float xn = cx * x + c0 * x0;
      if (c1 != 0.f) xn = fmaf(c1, x0h[i], xn);
      if (cn != 0.f) xn = fmaf(cn, z[j], xn);
      if (masked) {
        const float m = mask[(long long)b * HW + hw];
        const float kn = fmaf(ra, x0i[i], rn * z2[j]);
        xn = m * xn + (1.0f - m) * kn;
      }
      lat[i] = xn;
      x0h[i] = x0;
    }
  }
}

// The head's launch, and the argument rule of each of its four entries in front of it.
template <typename T>
static int latent_stack(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s) {
  const long long n = (long long)B * H * W * (C + Cc);
  void (*k)(T*, const float*, const float*, int, int, int, int, unsigned) =
      groups == 3 ? k_latent_stack<T, 3> : groups == 2 ? k_latent_stack<T, 2> : k_latent_stack<T, 1>;
  hipLaunchKernelGGL(k, dim3(ew_grid(n)), dim3(EW_BLOCK), 0, tf_hs(s), (T*)x_out, (const float*)latent, (const float*)cond, B, C, Cc, H * W, drop_bits);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

// what the two entries that take conditioning channels ask of the sizes and of x_out
static int stack_limits(const char* name, const void* x_out, int C, int Cc, int H, int W) {
  TF_REQUIRE((long long)H * W < (1LL << 31) && (long long)C + Cc < (1LL << 16), "%s: %lld pixels of %lld channels", name, (long long)H * W, (long long)C + Cc);
  TF_REQUIRE(((uintptr_t)x_out & 1) == 0, "%s: x_out must be 2-byte aligned", name);
  return TF_OK;
}

// the CFG pair of the latent alone; H == 0 or W == 0 is accepted and writes nothing
template <typename T>
static int cfg_duplicate(const char* name, void* x2b, const void* latent, int B, int C, int H, int W, tfStream_t s) {
  TF_REQUIRE(x2b && latent && B > 0 && C > 0 && H >= 0 && W >= 0, "%s: bad arguments", name);
  return latent_stack<T>(x2b, latent, nullptr, B, C, 0, H, W, 2, 0u, s);
}

// three guidance groups of the latent alone (perturbed-attention guidance on a 4-channel UNet): cfg_duplicate's rule, which tf_cfg_concat_* (Cc > 0,
// cond set) cannot express
template <typename T>
static int latent_stack3(const char* name, void* x3b, const void* latent, int B, int C, int H, int W, tfStream_t s) {
  TF_REQUIRE(x3b && latent && B > 0 && C > 0 && H >= 0 && W >= 0, "%s: bad arguments", name);
  return latent_stack<T>(x3b, latent, nullptr, B, C, 0, H, W, 3, 0u, s);
}

template <typename T>
static int cfg_concat(const char* name, void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits,
                      tfStream_t s) {
  TF_REQUIRE(x_out && latent && cond && B > 0 && C > 0 && Cc > 0 && H > 0 && W > 0, "%s: bad arguments (B=%d C=%d Cc=%d H=%d W=%d)", name, B, C, Cc, H, W);
  TF_REQUIRE(groups == 2 || groups == 3, "%s: groups=%d (2 or 3)", name, groups);
  if (const int e = stack_limits(name, x_out, C, Cc, H, W)) return e;
  return latent_stack<T>(x_out, latent, cond, B, C, Cc, H, W, groups, drop_bits, s);
}

template <typename T>
static int latent_stack1(const char* name, void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s) {
  TF_REQUIRE(x_out && latent && B > 0 && C > 0 && Cc >= 0 && H > 0 && W > 0, "%s: bad arguments (B=%d C=%d Cc=%d H=%d W=%d)", name, B, C, Cc, H, W);
  TF_REQUIRE((cond != nullptr) == (Cc > 0), "%s: cond is %s with Cc=%d (cond == NULL iff Cc == 0)", name, cond ? "set" : "NULL", Cc);
  if (const int e = stack_limits(name, x_out, C, Cc, H, W)) return e;
  return latent_stack<T>(x_out, latent, cond, B, C, Cc, H, W, 1, 0u, s);
}

// The tail's launch: the arguments every entry shares, then the instance of (G, mask set).  own_ptrs: the pointers only this entry requires
// are set (part of "bad arguments"); broken_rule: NULL, or the text of the entry's own rule that the arguments break.
template <typename T>
static int sampler_step(const char* name, int G, void* latent, const void* eps, void* x0_hist, const void* params, const void* coeffs, int rows, const void* edit,
                        const void* x0_init, const void* mask, bool own_ptrs, const char* broken_rule, int B, int C, int H, int W, tfStream_t s,
                        unsigned flags = 0u, const void* rescale = nullptr) {
  TF_REQUIRE(latent && eps && x0_hist && params && coeffs && own_ptrs && rows >= 1 && B > 0 && C > 0 && H > 0 && W > 0, "%s: bad arguments (rows=%d B=%d C=%d H=%d W=%d)",
             name, rows, B, C, H, W);
  TF_REQUIRE(!broken_rule, "%s: bad arguments (%s)", name, broken_rule);
  const long long n_img = (long long)C * H * W;
  TF_REQUIRE(n_img <= (1LL << 32), "%s: %lld elements per image exceed the 2^32 Philox counters of an image", name, n_img);
  if (flags & (TAIL_VPRED | TAIL_RESCALE)) {                      // (tf_sampler_tail_* alone sets flags)
    void (*kr)(float*, const T*, float*, const float*, const float*, int, const float*, const float*, const float*, const float*, int, int, int, unsigned) =
        G == 3 ? k_sampler_step_rescale<T, 3> : G == 2 ? k_sampler_step_rescale<T, 2> : k_sampler_step_rescale<T, 1>;
    long long grid = B;                                            // rescale: one block per image
    if (!(flags & TAIL_RESCALE)) {
      grid = ceil_div_ll(((n_img + 3) >> 2) * B, RS_BLOCK);
      if (grid > 512) grid = 512;                                  // (ew_grid's cap in threads)
    }
    hipLaunchKernelGGL(kr, dim3((unsigned)grid), dim3(RS_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps, (float*)x0_hist, (const float*)params, (const float*)coeffs,
                       rows, (const float*)edit, (const float*)x0_init, (const float*)mask, (const float*)rescale, B, C, H * W, flags);
    TF_LAUNCH_CHECK();
    return TF_OK;
  }
  void (*k)(float*, const T*, float*, const float*, const float*, int, const float*, const float*, const float*, int, int, int) =
      G == 3 ? (mask ? k_sampler_step<T, 3, true> : k_sampler_step<T, 3, false>)
      : G == 2 ? (mask ? k_sampler_step<T, 2, true> : k_sampler_step<T, 2, false>)
               : (mask ? k_sampler_step<T, 1, true> : k_sampler_step<T, 1, false>);
  hipLaunchKernelGGL(k, dim3(ew_grid(((n_img + 3) >> 2) * B)), dim3(EW_BLOCK), 0, tf_hs(s), (float*)latent, (const T*)eps, (float*)x0_hist, (const float*)params,
                     (const float*)coeffs, rows, (const float*)edit, (const float*)x0_init, (const float*)mask, B, C, H * W);
  TF_LAUNCH_CHECK();
  return TF_OK;
}

// tf_sampler_tail_*: the one entry that states every form by `groups` and `flags` (bit 0 v-prediction, bit 1 the masked blend, bit 2 CFG
// rescale); NULL, or the text of the first pointer / flag rule the arguments break
static inline const char* tail_rule(const void* edit, const void* x0_init, const void* mask, const void* rescale, int groups, unsigned flags) {
  if (groups < 1 || groups > 3) return "groups is 1, 2 or 3";
  if (flags & ~(unsigned)(TAIL_VPRED | TAIL_MASKED | TAIL_RESCALE)) return "flags has bits 0 (v-prediction), 1 (masked blend) and 2 (CFG rescale) only";
  const bool masked = (flags & TAIL_MASKED) != 0, resc = (flags & TAIL_RESCALE) != 0;
  if ((x0_init != nullptr) != masked || (mask != nullptr) != masked) return "x0_init and mask are both set iff flags bit 1 (the masked blend) is set";
  if ((edit != nullptr) != (groups == 3)) return "edit_params is set iff groups == 3";
  if ((rescale != nullptr) != resc) return "rescale is set iff flags bit 2 (CFG rescale) is set";
  if (resc && groups == 1) return "CFG rescale (flags bit 2) needs a text group next to another one: groups >= 2";
  return nullptr;
}

template <typename T>
static int sampler_tail(const char* name, void* latent, const void* eps, void* x0_hist, const void* params, const void* coeffs, int rows, const void* edit,
                        const void* x0_init, const void* mask, const void* rescale, int B, int C, int H, int W, int groups, unsigned flags, tfStream_t s) {
  const char* rule = tail_rule(edit, x0_init, mask, rescale, groups, flags);
  return sampler_step<T>(name, rule ? 1 : groups, latent, eps, x0_hist, params, coeffs, rows, edit, x0_init, mask, true, rule, B, C, H, W, s, rule ? 0u : flags,
                         rescale);
}

// tf_sampler_step1_*: both of x0_init and mask (the masked form) or neither
static inline const char* step1_rule(const void* x0_init, const void* mask) {
  return (x0_init != nullptr) == (mask != nullptr) ? nullptr : "x0_init and mask go together: both set for the masked form, both NULL for the plain one";
}

extern "C" {

int tf_randn_f32(void* out, int images, long long per_image, unsigned seed_lo, unsigned seed_hi, int image_offset, int step, int tag, tfStream_t s) {
  TF_REQUIRE(out && images >= 0 && per_image >= 0 && image_offset >= 0 && step >= 0 && tag >= 0, "tf_randn_f32: bad arguments (images=%d per_image=%lld offset=%d step=%d tag=%d)",
             images, per_image, image_offset, step, tag);
  TF_REQUIRE(per_image <= (1LL << 32), "tf_randn_f32: %lld elements per image exceed the 2^32 Philox counters of an image", per_image);
  if (images == 0 || per_image == 0) return TF_OK;
  hipLaunchKernelGGL(k_randn, dim3(ew_grid(((per_image + 3) >> 2) * images)), dim3(EW_BLOCK), 0, tf_hs(s), (float*)out, per_image, images, seed_lo, seed_hi,
                     (u32)image_offset, (u32)step, (u32)tag);
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
  hipLaunchKernelGGL(k_noise_to_level, dim3(ew_grid(((per_image + 3) >> 2) * images)), dim3(EW_BLOCK), 0, tf_hs(s), (float*)out, (const float*)x0,
                     per_image, images, a, seed_lo, seed_hi, (u32)image_offset);
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

int tf_cfg_duplicate_f16(void* x2b, const void* latent, int B, int C, int H, int W, tfStream_t s) {
  return cfg_duplicate<half_t>("tf_cfg_duplicate_f16", x2b, latent, B, C, H, W, s);
}

int tf_cfg_duplicate_bf16(void* x2b, const void* latent, int B, int C, int H, int W, tfStream_t s) {
  return cfg_duplicate<bf16_t>("tf_cfg_duplicate_bf16", x2b, latent, B, C, H, W, s);
}

int tf_cfg_concat_f16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s) {
  return cfg_concat<half_t>("tf_cfg_concat_f16", x_out, latent, cond, B, C, Cc, H, W, groups, drop_bits, s);
}

int tf_cfg_concat_bf16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, int groups, unsigned drop_bits, tfStream_t s) {
  return cfg_concat<bf16_t>("tf_cfg_concat_bf16", x_out, latent, cond, B, C, Cc, H, W, groups, drop_bits, s);
}

int tf_latent_stack1_f16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s) {
  return latent_stack1<half_t>("tf_latent_stack1_f16", x_out, latent, cond, B, C, Cc, H, W, s);
}

int tf_latent_stack1_bf16(void* x_out, const void* latent, const void* cond, int B, int C, int Cc, int H, int W, tfStream_t s) {
  return latent_stack1<bf16_t>("tf_latent_stack1_bf16", x_out, latent, cond, B, C, Cc, H, W, s);
}

int tf_cfg_sampler_step_f32(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<half_t>("tf_cfg_sampler_step_f32", 2, latent, eps2, x0_hist, params, coeffs, rows, nullptr, nullptr, nullptr, true, nullptr, B, C, H, W, s);
}

int tf_cfg_sampler_step_bf16(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<bf16_t>("tf_cfg_sampler_step_bf16", 2, latent, eps2, x0_hist, params, coeffs, rows, nullptr, nullptr, nullptr, true, nullptr, B, C, H, W, s);
}

int tf_cfg_sampler_step_masked_f32(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, const void* x0_init,
                                   const void* mask, int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<half_t>("tf_cfg_sampler_step_masked_f32", 2, latent, eps2, x0_hist, params, coeffs, rows, nullptr, x0_init, mask, x0_init && mask, nullptr, B, C,
                              H, W, s);
}

int tf_cfg_sampler_step_masked_bf16(void* latent, const void* eps2, void* x0_hist, const void* params, const void* coeffs, int rows, const void* x0_init,
                                    const void* mask, int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<bf16_t>("tf_cfg_sampler_step_masked_bf16", 2, latent, eps2, x0_hist, params, coeffs, rows, nullptr, x0_init, mask, x0_init && mask, nullptr, B, C,
                              H, W, s);
}

int tf_cfg3_sampler_step_f32(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                             int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<half_t>("tf_cfg3_sampler_step_f32", 3, latent, eps3, x0_hist, step_params, coeffs, rows, edit_params, nullptr, nullptr, edit_params != nullptr,
                              nullptr, B, C, H, W, s);
}

int tf_cfg3_sampler_step_bf16(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                              int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<bf16_t>("tf_cfg3_sampler_step_bf16", 3, latent, eps3, x0_hist, step_params, coeffs, rows, edit_params, nullptr, nullptr, edit_params != nullptr,
                              nullptr, B, C, H, W, s);
}

int tf_latent_stack3_f16(void* x3b, const void* latent, int B, int C, int H, int W, tfStream_t s) {
  return latent_stack3<half_t>("tf_latent_stack3_f16", x3b, latent, B, C, H, W, s);
}

int tf_latent_stack3_bf16(void* x3b, const void* latent, int B, int C, int H, int W, tfStream_t s) {
  return latent_stack3<bf16_t>("tf_latent_stack3_bf16", x3b, latent, B, C, H, W, s);
}

int tf_cfg3_sampler_step_masked_f32(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                                    const void* x0_init, const void* mask, int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<half_t>("tf_cfg3_sampler_step_masked_f32", 3, latent, eps3, x0_hist, step_params, coeffs, rows, edit_params, x0_init, mask,
                              edit_params && x0_init && mask, nullptr, B, C, H, W, s);
}

int tf_cfg3_sampler_step_masked_bf16(void* latent, const void* eps3, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                                     const void* x0_init, const void* mask, int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<bf16_t>("tf_cfg3_sampler_step_masked_bf16", 3, latent, eps3, x0_hist, step_params, coeffs, rows, edit_params, x0_init, mask,
                              edit_params && x0_init && mask, nullptr, B, C, H, W, s);
}

int tf_sampler_step1_f32(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init, const void* mask,
                         int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<half_t>("tf_sampler_step1_f32", 1, latent, eps, x0_hist, step_params, coeffs, rows, nullptr, x0_init, mask, true, step1_rule(x0_init, mask), B, C,
                              H, W, s);
}

int tf_sampler_step1_bf16(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* x0_init, const void* mask,
                          int B, int C, int H, int W, tfStream_t s) {
  return sampler_step<bf16_t>("tf_sampler_step1_bf16", 1, latent, eps, x0_hist, step_params, coeffs, rows, nullptr, x0_init, mask, true, step1_rule(x0_init, mask), B, C,
                              H, W, s);
}

int tf_sampler_tail_f32(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                        const void* x0_init, const void* mask, const void* rescale, int B, int C, int H, int W, int groups, unsigned flags, tfStream_t s) {
  return sampler_tail<half_t>("tf_sampler_tail_f32", latent, eps, x0_hist, step_params, coeffs, rows, edit_params, x0_init, mask, rescale, B, C, H, W, groups, flags, s);
}

int tf_sampler_tail_bf16(void* latent, const void* eps, void* x0_hist, const void* step_params, const void* coeffs, int rows, const void* edit_params,
                         const void* x0_init, const void* mask, const void* rescale, int B, int C, int H, int W, int groups, unsigned flags, tfStream_t s) {
  return sampler_tail<bf16_t>("tf_sampler_tail_bf16", latent, eps, x0_hist, step_params, coeffs, rows, edit_params, x0_init, mask, rescale, B, C, H, W, groups, flags, s);
}

}  // extern "C"
