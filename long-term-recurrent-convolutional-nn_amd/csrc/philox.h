// philox.h -- the counter-based generator and Gumbel noise of the sampled decode (lrcn_sample_batch, include/lrcn_sample.h).
// Philox4x32-10 (Salmon et al., SC'11): counter (col >> 2, current, s, i), key (seed & 0xffffffff, seed >> 32); column col uses word
// col & 3, so one call serves four neighbouring columns.  g = -log(-log(u)), u = ((x >> 9) + 0.5) * 2^-23 in float32: u lies in
// [2^-24, 1 - 2^-24] (both exact), g in [-2.812, 16.636] -- a column whose z / T is more than 19.45 below the row's max / T cannot win.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct Philox4 {
    uint32_t x[4];
};

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__host__ __device__ __forceinline__ float gumbel_of(uint32_t x) {
    const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}

// a column whose logit is below max - GUMBEL_PRUNE * T cannot be the argmax of z / T + g (19.45 would do; the rest is rounding slack)
#define GUMBEL_PRUNE 20.0f
