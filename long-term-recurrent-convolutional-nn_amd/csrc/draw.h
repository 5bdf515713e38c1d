// draw.h -- device code shared by the kernels that draw a word from a row of f32 logits with 256-thread workgroups: the sampled decode
// (sample.hip) and scheduled sampling's next-input kernel (train_kernels.hip).  (score, column) reductions over wave64 and the workgroup,
// and the Gumbel argmax over the admitted columns of a row, four columns (one Philox call) per thread and round.
#pragma once
#include "philox.h"

// (score, column) pairs: larger score first, lower column in a tie
__device__ __forceinline__ bool beats(float a, int ai, float b, int bi) { return a > b || (a == b && ai < bi); }
__device__ __forceinline__ void wave_best(float &v, int &i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (beats(ov, oi, v, i)) { v = ov; i = oi; }
    }
}
// block-wide best pair (256 threads); every thread gets the result
__device__ __forceinline__ void block_best(float &v, int &i, float *shv, int *shi) {
    wave_best(v, i);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[w] = v; shi[w] = i; }
    __syncthreads();
    v = shv[0]; i = shi[0];
    for (int q = 1; q < 4; ++q)
        if (beats(shv[q], shi[q], v, i)) { v = shv[q]; i = shi[q]; }
}
__device__ __forceinline__ float block_reduce(float v, float *sh, bool is_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = is_max ? fmaxf(v, __shfl_xor(v, o)) : v + __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return is_max ? fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) : (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// The row's maximum; stage != 0 also copies the row g[0, V) into srow (LDS), published by the reduction's barriers.
__device__ __forceinline__ float row_max_stage(const float *g, int V, int stage, float *srow, float *shf) {
    float m = -INFINITY;
    for (int j = threadIdx.x; j < V; j += 256) {
        const float x = g[j];
        if (stage) srow[j] = x;
        m = fmaxf(m, x);
    }
    return block_reduce(m, shf, true);
}

// This thread's best of argmax_j (z_j / temp + g_j) over its columns j (quads q = tid, tid + 256, ...) with z_j >= thr and admit(z_j, j):
// score bs, column bc, logit bz.  g_j = gumbel_of(word j & 3 of Philox counter (j >> 2, c1, c2, c3)); temp == 0: the score is z_j itself.
// The workgroup's winner is block_best of (bs, bc).
template <class Admit>
__device__ __forceinline__ void gumbel_argmax(const float *z, int V, float temp, float thr, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, const Admit &admit, float &bs, int &bc, float &bz) {
    bs = -INFINITY;
    bz = -INFINITY;
    bc = 0x7FFFFFFF;
    for (int q = threadIdx.x; 4 * q < V; q += 256) {
        float x[4];
        bool ok[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = 4 * q + k;
            x[k] = j < V ? z[j] : -INFINITY;
            ok[k] = j < V && x[k] >= thr && admit(x[k], j);
            any |= ok[k];
        }
        if (!any) continue;
        if (temp > 0.0f) {
            const Philox4 rnd = philox4x32_10((uint32_t)q, c1, c2, c3, k0, k1);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) {
                    const float sc = x[k] / temp + gumbel_of(rnd.x[k]);
                    if (beats(sc, 4 * q + k, bs, bc)) { bs = sc; bc = 4 * q + k; bz = x[k]; }
                }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k] && beats(x[k], 4 * q + k, bs, bc)) { bs = x[k]; bc = 4 * q + k; bz = x[k]; }
        }
    }
}
