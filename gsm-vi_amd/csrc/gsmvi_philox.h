// Counter-based Philox4x32-10 and the 53-bit uniform of the device draw stream (csrc/gsmvi_rng.hip), shared by every
// kernel that draws from it (k_randn; the batched fit step of gsmvi_batched.hip draws its next samples in place).  Element
// pair p of draw `call` under key `seed` is philox_normal_pair of philox4x32_10((p lo, p hi, call lo, call hi), (seed lo,
// seed hi)): one code path, so every kernel gives the same bits for the same (seed, call, p).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
        const unsigned n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        const unsigned n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 53-bit uniform in (0, 1): ((a >> 5) 2^26 + (b >> 6) + 1/2) 2^-53 -- never 0, never 1
__device__ __forceinline__ double u53(unsigned a, unsigned b) {
    const unsigned long long m = ((unsigned long long)(a >> 5) << 26) | (unsigned long long)(b >> 6);
    return ((double)m + 0.5) * (1.0 / 9007199254740992.0);
}

// Box-Muller of one Philox block: the element pair (z[2p], z[2p+1]) of the stream
__device__ __forceinline__ void philox_normal_pair(const unsigned (&w)[4], double& z0, double& z1) {
    const double u1 = u53(w[0], w[1]), u2 = u53(w[2], w[3]);
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    z0 = r * c;
    z1 = r * s;
}
