// kernels.hip -- the HBM-bound kernels that more than one model file launches: embedding gather, LSTM cell forward / backward, [x | cnn]
// concatenation with dropout, layout transposes, casts, column sums, fills (one wave = 64 lanes).  Beside it: xent.hip (the fused log-softmax +
// NLL + dlogits stage) and what one host file alone uses -- train_kernels.hip (train.hip, update.hip), decode_kernels.hip (decode.hip),
// image_kernels.hip (the VGG side).
#include "kernel_util.h"

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
__global__ void embed_gather_kernel(const T *wembT, int64_t ld_w, const int32_t *tok_in, int S, int B, int E, DropSpec d,
                                    T *xemb, int64_t ld_x) {
    const int m = blockIdx.x;
    const int s = m / B, b = m - s * B;
    const T *src = wembT + (int64_t)tok_in[m] * ld_w;
    T *dst = xemb + (int64_t)m * ld_x;
    for (int e = threadIdx.x; e < E; e += blockDim.x) dst[e] = from_f32<T>(to_f32(src[e]) * drop_mult(d, s, b, e, B, E));
}

template <typename T>
__global__ void lstm_fwd_kernel(const float *G, int64_t ld_g, const float *c_prev, int B, int H, T *acts, int64_t ld_a,
                                float *c_new, T *h_new, int64_t ld_h, float *h_new_f32) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= H) return;
    const float *g = G + (int64_t)b * ld_g;
    const float f = sigm(g[j]), i = sigm(g[H + j]), o = sigm(g[2 * H + j]), ch = tanhf(g[3 * H + j]);
    const float cp = c_prev ? c_prev[(int64_t)b * H + j] : 0.0f;
    const float c = cp * f + i * ch;
    const float h = o * tanhf(c);
    T *a = acts + (int64_t)b * ld_a;
    a[j] = from_f32<T>(f);
    a[H + j] = from_f32<T>(i);
    a[2 * H + j] = from_f32<T>(o);
    a[3 * H + j] = from_f32<T>(ch);
    c_new[(int64_t)b * H + j] = c;
    h_new[(int64_t)b * ld_h + j] = from_f32<T>(h);
    if (h_new_f32) h_new_f32[(int64_t)b * H + j] = h;
}

template <typename T>
__global__ void lstm_bwd_kernel(const T *acts, int64_t ld_a, const float *c_prev, const float *c_new, const float *dh_a,
                                int64_t ld_dha, float *dh_b, int dh_b_read, float *dc, int dc_zero, int B, int H, T *dz, int64_t ld_dz, int nslab) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (j >= H) return;
    const T *a = acts + (int64_t)b * ld_a;
    const float f = to_f32(a[j]), i = to_f32(a[H + j]), o = to_f32(a[2 * H + j]), g = to_f32(a[3 * H + j]);
    const float tc = tanhf(c_new[(int64_t)b * H + j]);
    float dh = dh_a[(int64_t)b * ld_dha + j];
    if (nslab > 0) {  // recurrent dh from step s+1 as the K slices' partial sums [nslab][B][H] of a split-K GEMM without a reduce launch, summed
        if (dh_b_read)  // here in slice order (fixed: deterministic); the slabs are overwritten whole by step s-1's GEMM, nothing to zero
            for (int q = 0; q < nslab; ++q) dh += dh_b[((int64_t)q * B + b) * H + j];
    } else if (dh_b) {  // recurrent dh from step s+1; left zeroed for the split-K GEMM that accumulates step s-1's into it
        if (dh_b_read) dh += dh_b[(int64_t)b * H + j];
        dh_b[(int64_t)b * H + j] = 0.0f;
    }
    const float dov = dh * tc;
    const float dcv = (dc_zero ? 0.0f : dc[(int64_t)b * H + j]) + dh * o * (1.0f - tc * tc);
    const float cp = c_prev ? c_prev[(int64_t)b * H + j] : 0.0f;
    T *z = dz + (int64_t)b * ld_dz;
    z[j] = from_f32<T>(dcv * cp * f * (1.0f - f));
    z[H + j] = from_f32<T>(dcv * g * i * (1.0f - i));
    z[2 * H + j] = from_f32<T>(dov * o * (1.0f - o));
    z[3 * H + j] = from_f32<T>(dcv * i * (1.0f - g * g));
    dc[(int64_t)b * H + j] = dcv * f;
}

template <typename T>
__global__ void concat_x2_kernel(T *x2, int64_t ld_x2, const float *xcnn, int64_t ld_xc, int S, int B, int nl, int nr, DropSpec d, int s0) {
    const int m = blockIdx.x;
    const int sl = m / B, b = m - sl * B, s = s0 + sl;
    T *row = x2 + (int64_t)m * ld_x2;
    for (int j = threadIdx.x; j < nl + nr; j += blockDim.x) {
        const float v = (j < nl) ? to_f32(row[j]) : xcnn[(int64_t)b * ld_xc + (j - nl)];
        row[j] = from_f32<T>(v * drop_mult(d, s, b, j, B, nl + nr));
    }
}

template <typename Tin, typename Tout>
__global__ void transpose_kernel(const Tin *in, int64_t ld_in, int R, int C, Tout *out, int64_t ld_out, int shift) {
    __shared__ float tile[32][33];
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty 0..7
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < C) ? to_f32(in[(int64_t)r * ld_in + c]) : 0.0f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < C && r < R) out[(int64_t)c * ld_out + r + shift] = from_f32<Tout>(tile[tx][i]);
    }
    if (shift > 0 && blockIdx.y == 0) {
        for (int i = ty; i < 32; i += 8) {
            const int c = c0 + i;
            if (c < C)
                for (int r = tx; r < shift; r += 32) out[(int64_t)c * ld_out + r] = from_f32<Tout>(0.0f);
        }
    }
    if (blockIdx.y == gridDim.y - 1) {  // zero the K-padding [R + shift, ld_out) of every output row
        for (int i = ty; i < 32; i += 8) {
            const int c = c0 + i;
            if (c < C)
                for (int r = R + shift + tx; r < ld_out; r += 32) out[(int64_t)c * ld_out + r] = from_f32<Tout>(0.0f);
        }
    }
}

template <typename T>
__global__ void cast_rows_kernel(const float *in, int64_t ld_in, int R, int C, T *out, int64_t ld_out) {
    const int r = blockIdx.y;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ld_out; c += gridDim.x * blockDim.x)
        out[(int64_t)r * ld_out + c] = from_f32<T>(c < C ? in[(int64_t)r * ld_in + c] : 0.0f);
}

template <typename T, int RG> __global__ __launch_bounds__(16 * RG) void colsum_kernel(const T *z, int64_t ld, int M, int N, int rows_per_slab, float *out) {
    // block = 64 columns (16 lanes x 4 elements, one 8/16-byte load each) x RG row groups over one slab of rows (blockIdx.y).
    // One slab: plain store (no zeroing, deterministic).  Several slabs: f32 atomics into an output the host zeroed.
    __shared__ float sh[RG][65];
    const int q = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 64 + 4 * q;
    const int m0 = blockIdx.y * rows_per_slab, m1 = min(M, m0 + rows_per_slab);
    struct alignas(4 * sizeof(T)) V4 { T e[4]; };
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < N) {  // ld % 4 == 0 and N <= ld: the whole quad is inside the row
#pragma unroll 4
        for (int m = m0 + rg; m < m1; m += RG) {
            const V4 v = *reinterpret_cast<const V4 *>(z + (int64_t)m * ld + c);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += to_f32(v.e[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[rg][4 * q + k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int cc = blockIdx.x * 64 + threadIdx.x;
        float t = 0.0f;
#pragma unroll
        for (int r = 0; r < RG; ++r) t += sh[r][threadIdx.x];
        if (cc < N) {
            if (gridDim.y == 1) out[cc] = t;
            else atomicAdd(out + cc, t);
        }
    }
}

template <typename T> __global__ __launch_bounds__(256) void transpose_multi_kernel(const TrPlan plan) {
    __shared__ float tile[64][65];
    int d = 0;
#pragma unroll
    for (int k = 1; k < TR_MAX; ++k)
        if (k < plan.n && (int)blockIdx.x >= plan.d[k].tile0) d = k;
    const TrDesc &P = plan.d[d];
    const T *src = reinterpret_cast<const T *>(P.src);
    T *dst = reinterpret_cast<T *>(P.dst);
    const int t = blockIdx.x - P.tile0;
    const int tc = (P.C + 63) / 64, tr = P.R > 0 ? (P.R + 63) / 64 : 1;
    const int ty = t / tc;
    const int r0 = ty * 64, c0 = (t % tc) * 64;
    const int q = threadIdx.x & 15, rr = threadIdx.x >> 4;
    struct alignas(4 * sizeof(T)) V4 { T e[4]; };
    const bool vin = (P.ld_src % 4) == 0 && (reinterpret_cast<uintptr_t>(src) % sizeof(V4)) == 0;
    const bool vout = (P.ld_dst % 4) == 0 && (P.shift % 4) == 0 && (reinterpret_cast<uintptr_t>(dst) % sizeof(V4)) == 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + rr + 16 * i, c = c0 + 4 * q;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < P.R && c < P.C) {
            if (vin && c + 3 < P.ld_src) {
                const V4 x = *reinterpret_cast<const V4 *>(src + (int64_t)r * P.ld_src + c);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = to_f32(x.e[k]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < P.C) v[k] = to_f32(src[(int64_t)r * P.ld_src + c + k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[rr + 16 * i][4 * q + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + rr + 16 * i;  // source column = destination row
        if (c >= P.C) continue;
        T *row = dst + (int64_t)c * P.ld_dst;
        const int r = r0 + 4 * q;
        if (vout && r + 3 < P.R) {
            V4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o.e[k] = from_f32<T>(tile[4 * q + k][rr + 16 * i]);
            *reinterpret_cast<V4 *>(row + P.shift + r) = o;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (r + k < P.R) row[P.shift + r + k] = from_f32<T>(tile[4 * q + k][rr + 16 * i]);
        }
        if (ty == 0)
            for (int x = q; x < P.shift; x += 16) row[x] = from_f32<T>(0.0f);
        if (ty == tr - 1)
            for (int64_t x = P.R + P.shift + q; x < P.ld_dst; x += 16) row[x] = from_f32<T>(0.0f);
    }
}

__global__ void init_uniform_kernel(float *w, int64_t n, float scale, uint64_t seed, int tensor) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t h = mix64(mix64(seed ^ ((uint64_t)(tensor + 1) * 0xD1342543DE82EF95ull)) ^ (uint64_t)i);
        const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);
        w[i] = (float)(2.0 * (double)scale * u - (double)scale);
    }
}
__global__ void fill_kernel(float *w, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) w[i] = v;
}

}  // namespace
// ---------------------------------------------------------------- launchers
void k_embed_gather(hipStream_t st, int dtype, const void *wembT, int64_t ld_w, const int32_t *tok_in, int S, int B, int E,
                    DropSpec d, void *xemb, int64_t ld_x) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(embed_gather_kernel<T>, dim3(S * B), dim3(256), 0, st, (const T *)wembT, ld_w,
                                         tok_in, S, B, E, d, (T *)xemb, ld_x));
}
void k_lstm_fwd(hipStream_t st, int dtype, const float *G, int64_t ld_g, const float *c_prev, int B, int H, void *acts,
                int64_t ld_a, float *c_new, void *h_new, int64_t ld_h, float *h_new_f32) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(lstm_fwd_kernel<T>, dim3(cdiv(H, 256), B), dim3(256), 0, st, G, ld_g, c_prev, B, H,
                                         (T *)acts, ld_a, c_new, (T *)h_new, ld_h, h_new_f32));
}
void k_lstm_bwd(hipStream_t st, int dtype, const void *acts, int64_t ld_a, const float *c_prev, const float *c_new,
                const float *dh_a, int64_t ld_dha, float *dh_b, int dh_b_read, float *dc, int dc_zero, int B, int H, void *dz, int64_t ld_dz, int nslab) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(lstm_bwd_kernel<T>, dim3(cdiv(H, 256), B), dim3(256), 0, st, (const T *)acts, ld_a,
                                         c_prev, c_new, dh_a, ld_dha, dh_b, dh_b_read, dc, dc_zero, B, H, (T *)dz, ld_dz, nslab));
}
void k_concat_x2(hipStream_t st, int dtype, void *x2, int64_t ld_x2, const float *xcnn, int64_t ld_xc, int S, int B, int nl, int nr,
                 DropSpec d, int s0) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(concat_x2_kernel<T>, dim3(S * B), dim3(256), 0, st, (T *)x2, ld_x2, xcnn, ld_xc, S,
                                         B, nl, nr, d, s0));
}
void k_transpose(hipStream_t st, int dtype, int in_f32, const void *in, int64_t ld_in, int R, int C, void *out,
                 int64_t ld_out, int shift) {
    const dim3 grid(cdiv(C, 32), cdiv(R, 32));
    DISPATCH_T(dtype, {
        if (in_f32)
            hipLaunchKernelGGL((transpose_kernel<float, T>), grid, dim3(256), 0, st, (const float *)in, ld_in, R, C, (T *)out,
                               ld_out, shift);
        else
            hipLaunchKernelGGL((transpose_kernel<T, T>), grid, dim3(256), 0, st, (const T *)in, ld_in, R, C, (T *)out, ld_out,
                               shift);
    });
}
void k_transpose_f32(hipStream_t st, const float *in, int64_t ld_in, int R, int C, float *out, int64_t ld_out) {
    hipLaunchKernelGGL((transpose_kernel<float, float>), dim3(cdiv(C, 32), cdiv(R, 32)), dim3(256), 0, st, in, ld_in, R, C,
                       out, ld_out, 0);
}
void k_cast_rows(hipStream_t st, int dtype, const float *in, int64_t ld_in, int R, int C, void *out, int64_t ld_out) {
    const dim3 grid(cdiv(ld_out, 256) > 64 ? 64 : cdiv(ld_out, 256), R);
    DISPATCH_T(dtype, hipLaunchKernelGGL(cast_rows_kernel<T>, grid, dim3(256), 0, st, in, ld_in, R, C, (T *)out, ld_out));
}
void k_colsum(hipStream_t st, int dtype, const void *z, int64_t ld, int M, int N, float *out, bool deterministic) {
    // enough slabs of rows to give the chip ~2 blocks per CU; a single slab needs no zeroing and no atomics
    const int cb = cdiv(N, 64);
    int slabs = (M <= 512 || deterministic) ? 1 : cdiv(512, cb);  // few rows: one pass, no memset launch (the step is launch-bound there)
    if (slabs > cdiv(M, 64)) slabs = cdiv(M, 64);
    if (slabs < 1) slabs = 1;
    const int rows = cdiv(cdiv(M, slabs), 16) * 16;
    slabs = cdiv(M, rows);
    if (slabs > 1) (void)hipMemsetAsync(out, 0, sizeof(float) * (size_t)N, st);
    if (slabs == 1 && deterministic && M > 512)  // the ordered form keeps one slab: 64 row groups per block instead of 16, summed in order
        DISPATCH_T(dtype, hipLaunchKernelGGL((colsum_kernel<T, 64>), dim3(cb, 1), dim3(1024), 0, st, (const T *)z, ld, M, N, rows, out));
    else
        DISPATCH_T(dtype, hipLaunchKernelGGL((colsum_kernel<T, 16>), dim3(cb, slabs), dim3(256), 0, st, (const T *)z, ld, M, N, rows, out));
}
void k_transpose_multi(hipStream_t st, int dtype, TrPlan &plan) {
    const int tiles = number_tiles(plan, 1);
    if (tiles == 0) return;
    DISPATCH_T(dtype, hipLaunchKernelGGL(transpose_multi_kernel<T>, dim3(tiles), dim3(256), 0, st, plan));
}
void k_init_uniform(hipStream_t st, float *w, int64_t n, float scale, uint64_t seed, int tensor) {
    hipLaunchKernelGGL(init_uniform_kernel, dim3(grid1d(n)), dim3(256), 0, st, w, n, scale, seed, tensor);
}
void k_fill(hipStream_t st, float *w, int64_t n, float v) {
    hipLaunchKernelGGL(fill_kernel, dim3(grid1d(n)), dim3(256), 0, st, w, n, v);
}
