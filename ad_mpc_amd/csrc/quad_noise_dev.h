// quad_noise_dev.h -- the counter-based generator of include/admpc_quad_noise.h as device text, for admpc_quad_plant.hip (the
// disturbances of a sub-step), admpc_quad_noise.hip (the same draws for the host) and quad_target_dev.h (the uniforms of a new target,
// which take the generator's calls at the far end of the fourth counter word).  Include INSIDE the translation unit's
// anonymous namespace; every function is __forceinline__.
#pragma once

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between them
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// call j of (vehicle b, period p, sub-step m) under key `seed`: the two words and the two normals of include/admpc_quad_noise.h, every
// operation rounded on its own
__device__ __forceinline__ void noise_pair(uint64_t seed, uint32_t b, uint64_t p, int m, int j, uint64_t& w0, uint64_t& w1, double& z0, double& z1)
{
#pragma clang fp contract(off)
    uint32_t o[4];
    philox4x32_10(b, (uint32_t)p, (uint32_t)(p >> 32), (uint32_t)(8 * m + j), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    w0 = (uint64_t)o[0] | (uint64_t)o[1] << 32;
    w1 = (uint64_t)o[2] | (uint64_t)o[3] << 32;
    const double u0 = ((double)(w0 >> 11) + 0.5) * 0x1p-53, u1 = ((double)(w1 >> 11) + 0.5) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u0)), a = 6.283185307179586 * u1;
    z0 = r * cos(a); z1 = r * sin(a);
}
