// score.hip -- the per-pair kernels of caption scoring (lrcn_score_matrix / lrcn_score_pairs, include/lrcn_score.h): s(n, m) = sum over the
// caption's steps of log softmax(z_t)[y_t].  The pair rows are caption-major and sorted by caption length, so the rows still active at step t
// are a prefix of the piece and every row keeps its state in place.  Per step:
//   score_prep_kernel        -- A2 row r = [P_t(caption of r) | h2] (the h2 block was written by the previous step's cell) and the row's target
//   score_gather_rows_kernel -- f32 rows of an input-projection table (T1 per token, U2 per image) for the unfused cell (lstm_fwd_kernel)
//   score_pick_merge_kernel  -- the GEMM_OUT_SMAX_PICK records of a row -> z[y] - max - log(sum exp), added to the row's double sum
//   score_acc_kernel         -- the same from k_softmax_xent's per-row terms (the unfused logits)
//   score_matrix_rows_kernel -- a matrix piece's row maps: row r = image r % N of sorted caption r / N
//   score_scatter_kernel     -- the finished sums to the caller's f32 scores
#include "kernels.h"

#include "common.h"
#include "gemm.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void score_prep_kernel(T *A2, int64_t ldA2, const T *P, int64_t ldP, const int32_t *row_cap, int R, int h,
                                                         int zero_h2, int64_t h2_off, const int32_t *tgt_cap, int32_t *tgt_row) {
    const int r = blockIdx.x;
    if (r >= R) return;
    const int j = row_cap[r];
    const T *src = P + (int64_t)j * ldP;
    T *dst = A2 + (int64_t)r * ldA2;
    for (int k = threadIdx.x; k < h; k += blockDim.x) dst[k] = src[k];
    if (zero_h2)
        for (int k = threadIdx.x; k < zero_h2; k += blockDim.x) dst[h2_off + k] = from_f32<T>(0.0f);
    if (threadIdx.x == 0) tgt_row[r] = tgt_cap[j];
}

__global__ __launch_bounds__(256) void score_gather_rows_kernel(const float *table, int C4, const int32_t *idx, int R, float *dst) {
    const int r = blockIdx.x;
    if (r >= R) return;
    const float4 *src = reinterpret_cast<const float4 *>(table) + (int64_t)idx[r] * C4;
    float4 *d = reinterpret_cast<float4 *>(dst) + (int64_t)r * C4;
    for (int k = threadIdx.x; k < C4; k += blockDim.x) d[k] = src[k];
}

// one wave per row: NR records per lane
template <int NR>
__global__ __launch_bounds__(256) void score_pick_merge_kernel(const float *part, int nrec, int R, double *acc) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;   // wave-uniform
    const float *rp = part + (int64_t)row * nrec * SMAX_REC;
    float m[NR], sx[NR];
    float gm = -INFINITY, zt = -INFINITY;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int rec = lane + 64 * q;
        m[q] = -INFINITY;
        sx[q] = 0.0f;
        if (rec < nrec) {
            const float4 a = *reinterpret_cast<const float4 *>(rp + (int64_t)rec * SMAX_REC);
            m[q] = a.x; sx[q] = a.y;
            zt = fmaxf(zt, a.z);   // exactly one record holds the target's logit, the others -inf
        }
        gm = fmaxf(gm, m[q]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gm = fmaxf(gm, __shfl_xor(gm, o));
        zt = fmaxf(zt, __shfl_xor(zt, o));
    }
    float se = 0.0f;
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (m[q] != -INFINITY) se += sx[q] * __expf(m[q] - gm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    if (lane == 0) acc[row] += (double)(zt - (gm + logf(se)));
}

__global__ void score_acc_kernel(const double *terms, int R, double *acc) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) acc[r] += terms[r];
}

__global__ void score_matrix_rows_kernel(int64_t r0, int R, int N, const int32_t *ord, int32_t *img, int32_t *cap, int32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    const int64_t r = r0 + i;
    const int j = (int)(r / N), n = (int)(r - (int64_t)j * N);
    img[i] = n;
    cap[i] = j;
    out[i] = n + ord[j] * N;   // (N * M < 2^31: checked by the caller)
}

__global__ void score_scatter_kernel(const double *acc, const int32_t *out_idx, int R, float *scores) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) scores[out_idx[r]] = (float)acc[r];
}

}  // namespace

void k_score_prep(hipStream_t st, int dtype, void *A2, int64_t ldA2, const void *P, int64_t ldP, const int32_t *row_cap, int R, int h, int zero_h2,
                  int64_t h2_off, const int32_t *tgt_cap, int32_t *tgt_row) {
    if (R <= 0) return;
    if (dtype == GEMM_T_BF16)
        hipLaunchKernelGGL(score_prep_kernel<bf16_t>, dim3(R), dim3(256), 0, st, reinterpret_cast<bf16_t *>(A2), ldA2,
                           reinterpret_cast<const bf16_t *>(P), ldP, row_cap, R, h, zero_h2, h2_off, tgt_cap, tgt_row);
    else
        hipLaunchKernelGGL(score_prep_kernel<float>, dim3(R), dim3(256), 0, st, reinterpret_cast<float *>(A2), ldA2,
                           reinterpret_cast<const float *>(P), ldP, row_cap, R, h, zero_h2, h2_off, tgt_cap, tgt_row);
}

void k_score_gather_rows(hipStream_t st, const float *table, int C, const int32_t *idx, int R, float *dst) {
    if (R <= 0) return;
    hipLaunchKernelGGL(score_gather_rows_kernel, dim3(R), dim3(256), 0, st, table, C / 4, idx, R, dst);
}

bool k_score_pick_merge(hipStream_t st, const float *part, int nrec, int R, double *acc) {
    if (R <= 0) return true;
    const dim3 grid((R + 3) / 4);
    if (nrec <= 64) hipLaunchKernelGGL(score_pick_merge_kernel<1>, grid, dim3(256), 0, st, part, nrec, R, acc);
    else if (nrec <= 128) hipLaunchKernelGGL(score_pick_merge_kernel<2>, grid, dim3(256), 0, st, part, nrec, R, acc);
    else if (nrec <= 256) hipLaunchKernelGGL(score_pick_merge_kernel<4>, grid, dim3(256), 0, st, part, nrec, R, acc);
    else return false;
    return true;
}

void k_score_acc(hipStream_t st, const double *terms, int R, double *acc) {
    if (R <= 0) return;
    hipLaunchKernelGGL(score_acc_kernel, dim3((R + 255) / 256), dim3(256), 0, st, terms, R, acc);
}

void k_score_matrix_rows(hipStream_t st, int64_t r0, int R, int N, const int32_t *ord, int32_t *img, int32_t *cap, int32_t *out) {
    if (R <= 0) return;
    hipLaunchKernelGGL(score_matrix_rows_kernel, dim3((R + 255) / 256), dim3(256), 0, st, r0, R, N, ord, img, cap, out);
}

void k_score_scatter(hipStream_t st, const double *acc, const int32_t *out_idx, int R, float *scores) {
    if (R <= 0) return;
    hipLaunchKernelGGL(score_scatter_kernel, dim3((R + 255) / 256), dim3(256), 0, st, acc, out_idx, R, scores);
}
