// xent.hip -- the loss stage of caption training and of the unfused caption scoring: fused log-softmax + NLL + d(logits), one workgroup
// per logits row, in five forms (kernels.h gives their formulas), and what goes with it -- the ordered sum of the per-row terms and the
// target check of lrcn_xent_logits.  One descriptor (XentCall), one launcher (k_softmax_xent).
#include "kernel_util.h"
#include <cassert>

namespace {

// The form of a call, derived by k_softmax_xent from its XentCall and nowhere else.  Each later form includes MASKED.
enum { XENT_PLAIN, XENT_MASKED, XENT_WEIGHTED, XENT_SMOOTH, XENT_SMOOTH_WEIGHTED };
template <int FORM> struct xent_form {
    static constexpr bool masked = FORM != XENT_PLAIN;
    static constexpr bool weighted = FORM == XENT_WEIGHTED || FORM == XENT_SMOOTH_WEIGHTED;
    static constexpr bool smooth = FORM == XENT_SMOOTH || FORM == XENT_SMOOTH_WEIGHTED;
};
// What only some forms read, by value behind the kernels' ten common arguments; a form loads the members it uses and no other.
struct XentTail {
    float eps;           // smooth
    const float *row_w;  // weighted: device f32 [B]
    int B;
    double *ll_sum;      // smooth: the accumulator of the unsmoothed terms, or NULL
    double *ll_rows;     // smooth: their per-row slots [M], or NULL
};

// LRCN_OPT_DETERMINISTIC: the loss is the sum of the per-row log p(target) taken by one workgroup in a fixed order
__global__ __launch_bounds__(256) void sum_rows_f64_kernel(const double *rows, int M, double *out) {
    __shared__ double sh[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < M; i += 256) a += rows[i];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out += sh[0];
}

// A row that the length-aware token builder marked inactive (target < 0: a step past its caption's end, include/lrcn_varlen.h) has no
// loss term: its logp_rows slot becomes exactly 0 and its dlog row all zeros (16-byte stores where the row allows), and its logits are
// never read.  The marker is uniform over the workgroup (one row per workgroup), so the early return crosses no barrier.
template <typename T>
__device__ __forceinline__ void softmax_xent_inactive_row(int m, int V, T *dlog, int64_t ld_d, double *logp_rows) {
    if (threadIdx.x == 0 && logp_rows) logp_rows[m] = 0.0;
    if (!dlog) return;
    T *drow = dlog + (int64_t)m * ld_d;
    constexpr int PER = 16 / (int)sizeof(T);
    int v = 0;
    if ((reinterpret_cast<uintptr_t>(drow) & 15) == 0) {
        const int nv = V / PER;
        for (int i = threadIdx.x; i < nv; i += blockDim.x) reinterpret_cast<uint4 *>(drow)[i] = make_uint4(0u, 0u, 0u, 0u);
        v = nv * PER;
    }
    for (int i = v + threadIdx.x; i < V; i += blockDim.x) drow[i] = from_f32<T>(0.0f);
}

// The start of row m: true for an inactive row, which is written here (the caller returns).  WEIGHTED (include/lrcn_weighted.h): the row
// belongs to caption b = m % B and carries the real weight w = row_w[b] -- zero makes it inactive (as uniform over the workgroup as the
// target's sign), any other value scales its d(logits) row and its terms.  With every weight 1.0f the arithmetic is the unweighted
// form's bit for bit (scale * 1.0f == scale).
// Two things here are for the compiler, and profiles/xent_call.md has what each is worth.  The result is true for the row that returns,
// and scale takes its weight before the test, not behind it: only then does the inactive row's code leave the kernel on a path of its
// own.  Otherwise its stores seem to reach the active row's re-read of tgt[m] and its row[t], two uniform loads that then cannot be shown
// unclobbered and become vector loads -- the first of them one that every wave waits for in front of its d(logits) stores.
template <typename T, int FORM>
__device__ __forceinline__ bool softmax_xent_row_skipped(int m, const int32_t *tgt, int V, T *dlog, int64_t ld_d, double *logp_rows,
                                                         const XentTail &tl, float &w, float &scale) {
    using F = xent_form<FORM>;
    if constexpr (F::weighted) {
        w = tl.row_w[m % tl.B];
        scale *= w;  // rs = scale * row_w[b], once per row
    }
    if constexpr (F::masked) {
        if (tgt[m] < 0 || (F::weighted && w == 0.0f)) {
            softmax_xent_inactive_row<T>(m, V, dlog, ld_d, logp_rows);
            if constexpr (F::smooth)
                if (threadIdx.x == 0 && tl.ll_rows) tl.ll_rows[m] = 0.0;
            return true;
        }
    }
    return false;
}

// Thread 0 of an active row emits its terms: zt the target's logit, mx the row's max, se = sum exp(z - mx), sd = sum (z - mx) (SMOOTH).
// SMOOTH (include/lrcn_smooth.h): ll = (z_t - max) - log se, u = sd / V - log se; the smoothed term goes where the other forms put
// theirs and the plain w * ll into the tail's second accumulator.
template <int FORM>
__device__ __forceinline__ void softmax_xent_emit(int m, float w, float zt, float mx, float se, float sd, int V, double *logp_sum,
                                                  double *logp_rows, const XentTail &tl) {
    using F = xent_form<FORM>;
    if constexpr (F::smooth) {
        const float lg = logf(se);
        const float ll = (zt - mx) - lg, u = sd / (float)V - lg;
        const double term = (double)w * ((1.0 - (double)tl.eps) * (double)ll + (double)tl.eps * (double)u);
        if (logp_rows) logp_rows[m] = term;
        else if (logp_sum) atomicAdd(logp_sum, term);
        if (tl.ll_rows) tl.ll_rows[m] = (double)w * (double)ll;
        else if (tl.ll_sum) atomicAdd(tl.ll_sum, (double)w * (double)ll);
    } else {
        const float ll = zt - (mx + logf(se));
        const double term = F::weighted ? (double)w * (double)ll : (double)ll;
        if (logp_rows) logp_rows[m] = term;
        else atomicAdd(logp_sum, term);
    }
}

// The streaming kernel: any V, any alignment, the row read three times.  SMOOTH: the target distribution is (1 - eps) onehot(t) + eps / V --
// one more block-wide sum, of (z_v - max), rides in the pass that forms the exponentials, and d(logits) loses eps / V everywhere and
// (1 - eps) at the target.
template <typename T, int FORM>
__global__ __launch_bounds__(256) void softmax_xent_kernel(const float *logits, int64_t ld_l, const int32_t *tgt, int M, int V, float scale,
                                                           double *logp_sum, T *dlog, int64_t ld_d, double *logp_rows, XentTail tl) {
    __shared__ float sh[8];
    constexpr bool SMOOTH = xent_form<FORM>::smooth;
    const int m = blockIdx.x;
    float w = 1.0f;
    if (softmax_xent_row_skipped<T, FORM>(m, tgt, V, dlog, ld_d, logp_rows, tl, w, scale)) return;
    const float *row = logits + (int64_t)m * ld_l;
    float mx = -INFINITY;
    for (int v = threadIdx.x; v < V; v += blockDim.x) mx = fmaxf(mx, row[v]);
    mx = block_max(mx, sh);
    float se = 0.0f;
    [[maybe_unused]] float sd = 0.0f;
    if constexpr (SMOOTH) {
        for (int v = threadIdx.x; v < V; v += blockDim.x) {
            const float d = row[v] - mx;
            sd += d;
            se += expf(d);
        }
        sd = block_sum(sd, sh);
    } else {
        for (int v = threadIdx.x; v < V; v += blockDim.x) se += expf(row[v] - mx);
    }
    se = block_sum(se, sh);
    const float lse = mx + logf(se);
    const int t = tgt[m];
    if (threadIdx.x == 0) softmax_xent_emit<FORM>(m, w, row[t], mx, se, sd, V, logp_sum, logp_rows, tl);
    if (dlog) {
        T *drow = dlog + (int64_t)m * ld_d;
        if constexpr (SMOOTH) {
            const float eps = tl.eps, on = 1.0f - eps, uv = eps / (float)V;
            for (int v = threadIdx.x; v < V; v += blockDim.x) {
                const float p = expf(row[v] - lse);
                drow[v] = from_f32<T>((p - (v == t ? on : 0.0f) - uv) * scale);
            }
        } else {
            for (int v = threadIdx.x; v < V; v += blockDim.x) {
                const float p = expf(row[v] - lse);
                drow[v] = from_f32<T>((p - (v == t ? 1.0f : 0.0f)) * scale);
            }
        }
    }
}

// The same for V <= 1024 Q with the row held in registers: one expf per element (e = expf(x - max), p = e / sum) instead of
// two, 16-byte loads; the log-likelihood term is unchanged (x[t] - (max + logf(sum))).
template <typename T, int Q, int FORM>
__global__ __launch_bounds__(256) void softmax_xent_reg_kernel(const float *logits, int64_t ld_l, const int32_t *tgt, int M, int V,
                                                               float scale, double *logp_sum, T *dlog, int64_t ld_d, double *logp_rows,
                                                               XentTail tl) {
    __shared__ float sh[8];
    constexpr bool SMOOTH = xent_form<FORM>::smooth;
    const int m = blockIdx.x;
    float w = 1.0f;
    if (softmax_xent_row_skipped<T, FORM>(m, tgt, V, dlog, ld_d, logp_rows, tl, w, scale)) return;
    const float *row = logits + (int64_t)m * ld_l;  // ld_l % 4 == 0, 16-byte aligned rows
    float x[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int v0 = 4 * (threadIdx.x + 256 * q);
        float4 f = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (v0 < V) f = *reinterpret_cast<const float4 *>(row + v0);
        x[q][0] = f.x;
        x[q][1] = v0 + 1 < V ? f.y : -INFINITY;
        x[q][2] = v0 + 2 < V ? f.z : -INFINITY;
        x[q][3] = v0 + 3 < V ? f.w : -INFINITY;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx = fmaxf(mx, x[q][j]);
    mx = block_max(mx, sh);
    float se = 0.0f;
    [[maybe_unused]] float sd = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (SMOOTH) {
                const float d = x[q][j] - mx;  // -inf for the padding: kept out of the sum
                if (4 * ((int)threadIdx.x + 256 * q) + j < V) sd += d;
                x[q][j] = expf(d);
            } else {
                x[q][j] = expf(x[q][j] - mx);  // 0 for the padding
            }
            se += x[q][j];
        }
    se = block_sum(se, sh);
    if constexpr (SMOOTH) sd = block_sum(sd, sh);
    const int t = tgt[m];
    if (threadIdx.x == 0) softmax_xent_emit<FORM>(m, w, row[t], mx, se, sd, V, logp_sum, logp_rows, tl);
    if (dlog) {
        T *drow = dlog + (int64_t)m * ld_d;
        const float inv = 1.0f / se;
        [[maybe_unused]] float on = 1.0f, uv = 0.0f;  // SMOOTH: what the target column and every column lose
        if constexpr (SMOOTH) {
            on = 1.0f - tl.eps;
            uv = tl.eps / (float)V;
        }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int v0 = 4 * (threadIdx.x + 256 * q);
            if (v0 >= V) continue;
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (SMOOTH) o[j] = (x[q][j] * inv - (v0 + j == t ? on : 0.0f) - uv) * scale;
                else o[j] = (x[q][j] * inv - (v0 + j == t ? 1.0f : 0.0f)) * scale;
            }
            if (v0 + 3 < V && (ld_d % 4) == 0) {
                store4(drow + v0, o);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (v0 + j < V) drow[v0 + j] = from_f32<T>(o[j]);
            }
        }
    }
}

__global__ void xent_targets_kernel(const int32_t *tgt, int M, int V, int32_t *out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < M) out[m] = (tgt[m] >= 0 && tgt[m] < V) ? tgt[m] : -1;
}

// One form's kernels: the register form up to V = 16384 on aligned rows (the rung Q = 2, 4, 8, 12, 16 that holds V), else the streaming one.
template <typename T, int FORM> void launch_softmax_xent(hipStream_t st, const XentCall &x, const XentTail &tl) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(x.M), dim3(256), 0, st, x.logits, x.ld_l, x.tgt, x.M, x.V, x.scale, x.sum, (T *)x.dlog, x.ld_d, x.rows, tl);
    };
    const bool reg = x.V <= 16384 && (x.ld_l % 4) == 0 && (reinterpret_cast<uintptr_t>(x.logits) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(x.dlog) & 15) == 0;
    const int q = (x.V + 1023) / 1024;
    if (!reg) go(softmax_xent_kernel<T, FORM>);
    else if (q <= 2) go(softmax_xent_reg_kernel<T, 2, FORM>);
    else if (q <= 4) go(softmax_xent_reg_kernel<T, 4, FORM>);
    else if (q <= 8) go(softmax_xent_reg_kernel<T, 8, FORM>);
    else if (q <= 12) go(softmax_xent_reg_kernel<T, 12, FORM>);
    else go(softmax_xent_reg_kernel<T, 16, FORM>);
}

}  // namespace

void k_softmax_xent(hipStream_t st, int dtype, const XentCall &x) {
    assert(x.masked || (!x.row_w && !(x.eps > 0.0f)));  // weights and smoothing are forms of the masked kernels
    assert(x.sum || x.rows || x.eps > 0.0f);            // only the smooth forms leave a NULL destination out
    const XentTail tl{x.eps, x.row_w, x.B, x.ll_sum, x.ll_rows};
    const int form = x.eps > 0.0f ? (x.row_w ? XENT_SMOOTH_WEIGHTED : XENT_SMOOTH) : x.row_w ? XENT_WEIGHTED : x.masked ? XENT_MASKED : XENT_PLAIN;
    DISPATCH_T(dtype, {
        switch (form) {
        case XENT_PLAIN: launch_softmax_xent<T, XENT_PLAIN>(st, x, tl); break;
        case XENT_MASKED: launch_softmax_xent<T, XENT_MASKED>(st, x, tl); break;
        case XENT_WEIGHTED: launch_softmax_xent<T, XENT_WEIGHTED>(st, x, tl); break;
        case XENT_SMOOTH: launch_softmax_xent<T, XENT_SMOOTH>(st, x, tl); break;
        default: launch_softmax_xent<T, XENT_SMOOTH_WEIGHTED>(st, x, tl); break;
        }
    });
    if (x.rows && x.sum) hipLaunchKernelGGL(sum_rows_f64_kernel, dim3(1), dim3(256), 0, st, x.rows, x.M, x.sum);
    if (x.ll_rows && x.ll_sum) hipLaunchKernelGGL(sum_rows_f64_kernel, dim3(1), dim3(256), 0, st, x.ll_rows, x.M, x.ll_sum);
}
void k_xent_targets(hipStream_t st, const int32_t *tgt, int M, int V, int32_t *out) {
    hipLaunchKernelGGL(xent_targets_kernel, dim3(cdiv(M, 256)), dim3(256), 0, st, tgt, M, V, out);
}
