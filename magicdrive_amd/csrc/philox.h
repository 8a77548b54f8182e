// philox.h — the device-side Gaussian noise the kernels of noise.hip share: Philox4x32-10 and the Box-Muller map of its words.
// ONE copy of each (as latent.h holds the x_in refresh): renoise_kernel and ddim_eta_kernel differ in the counter they pass only.
// A stream is named by counter word 3 (its domain): 0 = the forward jumps of mdx_latent_renoise_*, 1 = the variance noise of
// mdx_cfg_ddim_eta_step_*.  Two domains never share a block, whatever the seed, the element and counter word 2 are: Philox is a
// bijection of the counter for a fixed key.  include/mdx.h spells the mapping out to the bit.
#pragma once
#include "common.h"

namespace mdx {

#define MDX_NOISE_DOMAIN_RENOISE 0u
#define MDX_NOISE_DOMAIN_DDIM_ETA 1u

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned w[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// u1 = ((wa >> 8) + 1) 2^-24 in (0, 1], u2 = (wb >> 8) 2^-24 in [0, 1), both exact; (za, zb) = sqrt(-2 ln u1) (cos, sin)(2 pi u2)
__device__ __forceinline__ void box_muller(unsigned wa, unsigned wb, float& za, float& zb) {
    const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f, u2 = (float)(wb >> 8) * 0x1p-24f;
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    za = rad * cs; zb = rad * sn;
}

// z[0..3] of block k (relative elements 4k .. 4k + 3) of the group seeded `seed`, at counter word 2 = `visit`, in `domain`
__device__ __forceinline__ void noise_block(unsigned long long seed, long k, unsigned visit, unsigned domain, float z[4]) {
    unsigned w[4];
    philox4x32_10((unsigned)(unsigned long long)k, (unsigned)((unsigned long long)k >> 32), visit, domain, (unsigned)seed, (unsigned)(seed >> 32), w);
    box_muller(w[0], w[1], z[0], z[1]);
    box_muller(w[2], w[3], z[2], z[3]);
}

}  // namespace mdx
