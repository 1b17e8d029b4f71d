// psh_philox.h -- the counter-based generator psh_pdv.hip, psh_mrw.hip and psh_smrw.hip share: Random123's
// Philox4x32-10 keyed by the 64-bit seed (key = (seed lo, seed hi)), the two 53-bit words of one call, and Box-Muller on
// them.  The numpy twin is
// shadowing_amd/pdv.py (philox4x32_10, normal_pairs).
//   counter (c0, c1, g lo, g hi) gives the 64-bit words a = (x1:x0) >> 11 and b = (x3:x2) >> 11;
//   u1 = (a + 1) 2^-53 in (0, 1], u2 = b 2^-53 in [0, 1); rad = sqrt(-2 ln u1), z0 = rad cos(2 pi u2), z1 = rad sin(2 pi u2).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace psh {

#define PSH_TWO_PI 6.283185307179586

// Random123's Philox4x32-10 (the round of rocrand_philox4x32_10.h)
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    }
}

// the two 53-bit words of one Philox call on counter (c0, c1, g lo, g hi)
__device__ __forceinline__ void philox_words(uint32_t c0, uint32_t c1, uint64_t g, uint32_t k0, uint32_t k1, uint64_t& a,
                                             uint64_t& b) {
    uint32_t c2 = (uint32_t)g, c3 = (uint32_t)(g >> 32);
    philox4x32_10(c0, c1, c2, c3, k0, k1);
    a = ((((uint64_t)c1) << 32) | c0) >> 11;
    b = ((((uint64_t)c3) << 32) | c2) >> 11;
}

// one Box-Muller pair from counter (c0, c1, g lo, g hi)
__device__ __forceinline__ void philox_normal_pair(uint32_t c0, uint32_t c1, uint64_t g, uint32_t k0, uint32_t k1,
                                                   double& z0, double& z1) {
    uint64_t a, b;
    philox_words(c0, c1, g, k0, k1, a, b);
    const double u1 = (double)(a + 1) * 0x1p-53, u2 = (double)b * 0x1p-53;
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = PSH_TWO_PI * u2;
    double sn, cs;
    sincos(ang, &sn, &cs);       // the bits of sin(ang) and cos(ang), from one argument reduction instead of two
    z0 = rad * cs;
    z1 = rad * sn;
}

}  // namespace psh
