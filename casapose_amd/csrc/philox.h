// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): a counter-based generator, so any
// thread can draw the numbers of any (key, counter) without state.  The input pipeline (augment.hip) keys it with a per-image seed and counts
// (op slot, pixel, channel, 0): a halo pixel recomputed by a neighbouring tile draws exactly what its owner draws, and results do not depend
// on tiling, launch shape or shard.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CP_PHILOX_HD __host__ __device__ __forceinline__
#else   // a plain host compiler (csrc/scenes_selftest.cpp)
#define CP_PHILOX_HD inline
#endif

#include <cstdint>

namespace cp {

struct philox4 {
    uint32_t v[4];
};

CP_PHILOX_HD philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint64_t key) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return philox4{{c0, c1, c2, c3}};
}

// uniform in the open interval (0, 1) from 24 bits
CP_PHILOX_HD float u01(uint32_t x) { return (float)(x >> 8) * (1.f / 16777216.f) + (0.5f / 16777216.f); }

}  // namespace cp
