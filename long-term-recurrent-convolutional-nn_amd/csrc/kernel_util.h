// kernel_util.h -- internal to kernels.hip, xent.hip, train_kernels.hip, decode_kernels.hip, image_kernels.hip and activity.hip, what they share: the element-type
// dispatch, the dropout counter hash, wave / block reductions, the 4-element store and the launchers' grid helpers.
#pragma once
#include "kernels.h"
#include "common.h"
#include "gemm.h"

#define DISPATCH_T(dtype, ...)                    \
    do {                                          \
        if ((dtype) == GEMM_T_BF16) {             \
            using T = bf16_t;                     \
            __VA_ARGS__;                          \
        } else {                                  \
            using T = float;                      \
            __VA_ARGS__;                          \
        }                                         \
    } while (0)

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float hash_uniform(uint64_t seed, uint64_t stream, uint64_t idx) {
    const uint64_t h = mix64(mix64(seed ^ (stream * 0xD1342543DE82EF95ull)) ^ idx);
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}
// Dropout multiplier of element (s, b, j) of a (T+1) x [B x ncols] tensor  (Knet dropout: x .* (rand .> p) ./ (1-p)).
__device__ __forceinline__ float drop_mult(const DropSpec &d, int s, int b, int j, int B, int ncols) {
    if (d.mask) return d.mask[((int64_t)s * ncols + j) * B + b];
    if (d.p <= 0.0f) return 1.0f;
    const uint64_t idx = ((uint64_t)s * B + b) * (uint64_t)ncols + j;
    return hash_uniform(d.seed, (uint64_t)d.which, idx) > d.p ? 1.0f / (1.0f - d.p) : 0.0f;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float block_max(float v, float *sh) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = sh[0];
    for (int i = 1; i < nw; ++i) r = fmaxf(r, sh[i]);
    return r;
}
__device__ __forceinline__ float block_sum(float v, float *sh) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    float r = 0.0f;
    for (int i = 0; i < nw; ++i) r += sh[i];
    return r;
}

template <typename T> __device__ __forceinline__ void store4(T *p, const float *v) {
    struct alignas(4 * sizeof(T)) V4 { T e[4]; };
    V4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o.e[k] = from_f32<T>(v[k]);
    *reinterpret_cast<V4 *>(p) = o;
}

static inline unsigned grid1d(int64_t n, int block = 256, int64_t cap = 8192) {
    int64_t g = (n + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// Numbers the 64 x 64 tiles of a plan's descriptors in order (d[k].tile0 = the tiles before descriptor k) and returns their sum.
// min_row_tiles: what a descriptor without rows counts as (k_transpose_multi: 1, its C destination rows are zero-filled; else 0).
template <typename Plan> static int number_tiles(Plan &plan, int min_row_tiles) {
    int tiles = 0;
    for (int k = 0; k < plan.n; ++k) {
        plan.d[k].tile0 = tiles;
        tiles += std::max(cdiv(plan.d[k].R, 64), min_row_tiles) * cdiv(plan.d[k].C, 64);
    }
    return tiles;
}
