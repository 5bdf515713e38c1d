// ensemble.hip -- the mixture row of an ensemble decode step (include/lrcn_ensemble.h): M members' f32 logit rows in, one f32 row out that
// the constrained top-K kernel (constrain.hip) then reads as it reads one model's logits.  One workgroup of 256 per row; the members' row
// pointers, leading dimensions and weights arrive by value (EnsembleMixArgs), so a step uploads nothing and waits for nothing.
#include "kernel_util.h"

namespace {

// Four columns v0 .. v0 + 3 of a row.  `vec` (block-uniform: the row's base and leading dimension keep every group 16-byte aligned) and a
// whole group inside the row: one 16-byte load.  Else scalar loads of the columns below V only -- nothing is read at or past column V.
__device__ __forceinline__ void load4(const float *row, int v0, int V, bool vec, float pad, float x[4]) {
    if (vec && v0 + 3 < V) {
        const float4 f = *reinterpret_cast<const float4 *>(row + v0);
        x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = v0 + j < V ? row[v0 + j] : pad;
    }
}

// Pass 1: every member's (max, sum exp) over the row -- per thread a running pair over its column groups tid, tid + 256, ... in that order,
// then block_max and block_sum of the rescaled sums: lp_m[v] = (z_m[v] - max_m) - log(sum_m), the arithmetic family of
// softmax_topk_rows_kernel<Q, true> (__expf, __logf).  Pass 2: per column group the members' lp, combined as lrcn_ensemble.h defines
//   LOG_MEAN   x = sum_m w_m lp_m                                   (member order)
//   else       x = mx + log(sum_m w_m exp(lp_m - mx)), mx = max_m lp_m   (member order)
// and stored.  The second read of the members' rows (V * M * 4 bytes per workgroup, 340 KB at V = 10640 and M = 8) comes from L2 while the
// resident workgroups' rows fit it, else from the Infinity Cache or HBM (5120 x 10640: profiles/ensemble_bench.md).
// The member loops are unrolled to kEnsembleMax with m < M as a block-uniform predicate, so every per-member value lives in a register;
// vmask bit m: member m takes 16-byte loads, bit kEnsembleMax: `out` takes 16-byte stores.  No atomics: a call repeats bit for bit.
// One column group per thread and iteration: a form that loads four groups (pass 1) and two groups of every member (pass 2) ahead of
// their use took 115 VGPRs instead of 82 (4 waves per SIMD instead of 5) and lost its A/B at 5120 x 10640 (profiles/ensemble_bench.md).
template <bool LOG_MEAN>
__global__ __launch_bounds__(256) void ensemble_mix_rows_kernel(EnsembleMixArgs a, unsigned vmask, int V, float *out, int64_t ld_out) {
    __shared__ float sh[8];
    const int r = blockIdx.x, ngroup = (V + 3) >> 2;
    float mxm[kEnsembleMax], lsm[kEnsembleMax];
#pragma unroll
    for (int m = 0; m < kEnsembleMax; ++m) {
        mxm[m] = 0.0f;
        lsm[m] = 0.0f;
        if (m < a.M) {
            const float *row = a.z[m] + (int64_t)r * a.ld[m];
            const bool vec = (vmask >> m) & 1u;
            float tm = -INFINITY, ts = 0.0f;
            for (int g = threadIdx.x; g < ngroup; g += 256) {
                float x[4];
                load4(row, 4 * g, V, vec, -INFINITY, x);
                const float nm = fmaxf(tm, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));   // finite: column 4 g exists
                ts = ts * __expf(tm - nm) + ((__expf(x[0] - nm) + __expf(x[1] - nm)) + (__expf(x[2] - nm) + __expf(x[3] - nm)));
                tm = nm;
            }
            const float bm = block_max(tm, sh);
            // a thread without a column: tm = -inf, ts = 0, and exp(-inf) = 0
            const float bs = block_sum(ts * __expf(tm - bm), sh);
            mxm[m] = bm;
            lsm[m] = __logf(bs);
        }
    }
    float *orow = out + (int64_t)r * ld_out;
    const bool ovec = (vmask >> kEnsembleMax) & 1u;
    for (int g = threadIdx.x; g < ngroup; g += 256) {
        const int v0 = 4 * g;
        float lp[kEnsembleMax][4];
#pragma unroll
        for (int m = 0; m < kEnsembleMax; ++m)
            if (m < a.M) {
                float x[4];
                load4(a.z[m] + (int64_t)r * a.ld[m], v0, V, (vmask >> m) & 1u, 0.0f, x);
#pragma unroll
                for (int j = 0; j < 4; ++j) lp[m][j] = (x[j] - mxm[m]) - lsm[m];
            }
        float y[4];
        if (LOG_MEAN) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.0f;
#pragma unroll
                for (int m = 0; m < kEnsembleMax; ++m)
                    if (m < a.M) s += a.w[m] * lp[m][j];
                y[j] = s;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float mx = lp[0][j];
#pragma unroll
                for (int m = 1; m < kEnsembleMax; ++m)
                    if (m < a.M) mx = fmaxf(mx, lp[m][j]);
                float s = 0.0f;
#pragma unroll
                for (int m = 0; m < kEnsembleMax; ++m)
                    if (m < a.M) s += a.w[m] * __expf(lp[m][j] - mx);
                y[j] = mx + __logf(s);
            }
        }
        if (ovec && v0 + 3 < V) {
            *reinterpret_cast<float4 *>(orow + v0) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (v0 + j < V) orow[v0 + j] = y[j];
        }
    }
}

}  // namespace

void k_ensemble_mix_rows(hipStream_t st, const EnsembleMixArgs &a, bool log_mean, int R, int V, float *out, int64_t ld_out) {
    auto vec_ok = [](const void *p, int64_t ld) { return !(reinterpret_cast<uintptr_t>(p) & 15) && !(ld & 3); };
    unsigned vmask = vec_ok(out, ld_out) ? 1u << kEnsembleMax : 0u;
    for (int m = 0; m < a.M; ++m)
        if (vec_ok(a.z[m], a.ld[m])) vmask |= 1u << m;
    if (log_mean)
        hipLaunchKernelGGL((ensemble_mix_rows_kernel<true>), dim3(R), dim3(256), 0, st, a, vmask, V, out, ld_out);
    else
        hipLaunchKernelGGL((ensemble_mix_rows_kernel<false>), dim3(R), dim3(256), 0, st, a, vmask, V, out, ld_out);
}
