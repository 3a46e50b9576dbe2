// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011, "Parallel random numbers: as easy as 1, 2,
// 3"), the counter-based generator of the samplers (pb_sampler.hip, pb_nested.hip;
// sampler.philox_host is the same statement in NumPy): a pure function of (counter, key), so that
// host and device draw the same random words bit for bit and nothing has to be kept between
// launches.
//
// Addressing: key = the 64-bit seed (low word, high word); counter = (block, chain, generation,
// tag).  One block of four words gives two uniforms (words 0, 1 and words 2, 3) and, by Box-Muller
// from those two, two normals.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace pb {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
// what a block is drawn for (counter word 3): the sampler's three, then nested sampling's
constexpr uint32_t kTagPropose = 0, kTagAccept = 1, kTagInitial = 2;
constexpr uint32_t kTagNestedStart = 3, kTagNestedStep = 4, kTagNestedResample = 5;

struct PhiloxWords {
    uint32_t x[4];
};

__host__ __device__ inline PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                      uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0;
        const uint64_t p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return PhiloxWords{{c0, c1, c2, c3}};
}

// the block `block` of (chain, generation, tag) under the seed
__host__ __device__ inline PhiloxWords philox_block(uint64_t seed, uint32_t block, uint32_t chain,
                                                     uint32_t generation, uint32_t tag)
{
    return philox4x32_10(block, chain, generation, tag, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// 52 bits of two words -> a uniform in [2^-53, 1 - 2^-53]: (n + 0.5) 2^-52 with n < 2^52 is exact
__host__ __device__ inline double philox_u01(uint32_t hi, uint32_t lo)
{
    const uint64_t n = ((uint64_t)(hi >> 6) << 26) + (uint64_t)(lo >> 6);
    return ((double)n + 0.5) * 0x1p-52;
}

// the two uniforms of a block
__host__ __device__ inline void philox_block_uniforms(uint64_t seed, uint32_t block,
                                                      uint32_t chain, uint32_t generation,
                                                      uint32_t tag, double &ua, double &ub)
{
    const PhiloxWords r = philox_block(seed, block, chain, generation, tag);
    ua = philox_u01(r.x[0], r.x[1]);
    ub = philox_u01(r.x[2], r.x[3]);
}

// an index into n rows
__host__ __device__ inline int64_t philox_index(double u, int64_t n)
{
    const int64_t i = (int64_t)floor(u * (double)n);
    return i < n - 1 ? i : n - 1;
}

}  // namespace pb
