// The device normal generator of csrc/sampler.hip: Philox4x32-10 (Salmon et al. 2011, Random123), key = the 64-bit seed, counter = (q, global
// image index, step, tag); the q-th counter of an image gives its NCHW elements 4q .. 4q+3 through two Box-Muller pairs.  The tags are
// listed at the top of csrc/sampler.hip.
#pragma once
#include "common.h"

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, u32 k0, u32 k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const u32 hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const u32 hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
  }
  return c;
}
// u = ((bits >> 8) + 0.5) 2^-24 in (0, 1); z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1).  float64 inside: u near 1 has
// no fp32 image (the radius would round to 0), and a few hundred thousand latent elements per step make the cost irrelevant
__device__ __forceinline__ void box_muller(u32 a, u32 b, float& z0, float& z1) {
  const double u0 = ((double)(a >> 8) + 0.5) * 0x1p-24, u1 = ((double)(b >> 8) + 0.5) * 0x1p-24;
  const double r = sqrt(-2.0 * log(u0));
  double s, c;
  sincospi(2.0 * u1, &s, &c);
  z0 = (float)(r * c);
  z1 = (float)(r * s);
}
__device__ __forceinline__ void normal4(u32 k0, u32 k1, u32 q, u32 image, u32 step, u32 tag, float z[4]) {
  const uint4 v = philox4x32_10(make_uint4(q, image, step, tag), k0, k1);
  box_muller(v.x, v.y, z[0], z[1]);
  box_muller(v.z, v.w, z[2], z[3]);
}
