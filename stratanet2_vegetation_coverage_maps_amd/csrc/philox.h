// philox.h -- Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11) as include/strata_hip.h states it under sn2_subsample:
// counter (i, c1, key.lo, key.hi), key (seed.lo, seed.hi) -> the four output words.  sample.hip draws the subsample from the
// words of c1 = 0, feed.hip the augmentation of a training batch from c1 = 1, 2, 3.  Integer arithmetic only.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void sn2_philox4(unsigned long long seed, long long key, unsigned i, unsigned dom, unsigned w[4]) {
    unsigned c0 = i, c1 = dom, c2 = (unsigned)(unsigned long long)key, c3 = (unsigned)((unsigned long long)key >> 32);
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// u(seed, key, i) of sn2_subsample: the first two words of domain 0, the first one on top
__device__ __forceinline__ unsigned long long sn2_philox_u(unsigned long long seed, long long key, unsigned i) {
    unsigned w[4];
    sn2_philox4(seed, key, i, 0u, w);
    return ((unsigned long long)w[0] << 32) | w[1];
}
