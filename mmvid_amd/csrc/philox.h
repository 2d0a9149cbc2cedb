// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") and the word-to-variate mappings: the one statement of
// the counter-based generator behind the front end's training draws (frontend.hip) and the samplers' seeded race variates
// (variates.hip).  Host replicas: tests/frontend_ref.py (pinned to the Random123 known answers) and tests/variates_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct U4 {
    uint32_t x, y, z, w;
};
static __device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1,
                       n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}
static __device__ __forceinline__ float u01(uint32_t v) { return (float)(v >> 8) * (1.0f / 16777216.0f); }  // [0, 1)
// Exp(1): the argument ((v >> 8) + 1) * 2^-24 is an exact fp32 in (0, 1], so the result lies in [0, 24 ln 2] and is never inf or NaN
// (0.0f - x: +0 at the argument 1)
static __device__ __forceinline__ float exp1(uint32_t v) { return 0.0f - logf((float)((v >> 8) + 1u) * (1.0f / 16777216.0f)); }
