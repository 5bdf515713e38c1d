// sample.hip -- the per-step choice of the sampled decode (lrcn_sample_batch, include/lrcn_sample.h; the sample() path of lrcn.jl:613-621,
// 680-687).  Every row r = i * S + s of the batched step is its own hypothesis: it draws tok = argmax_j (z_j / T + g_j) over the whole
// vocabulary or its top_k largest logits (Gumbel-max: the draw has the distribution softmax(z / T)), appends it to its history and adds
// log softmax(z)[tok] (temperature 1) to its log-likelihood.  g_j comes from philox.h.  One form per route of the step:
//   sample_rows_kernel          -- from the f32 logits of a plain logits GEMM (any T, top_k <= 32, f32 contexts, LRCN_DECODE_SMAX=0)
//   sample_topk_merge_kernel    -- from the GEMM_OUT_SMAX_TOPK records (top_k < SMAX_KC): the row's top_k columns, noise for those only
//   sample_gumbel_merge_kernel  -- from the GEMM_OUT_SMAX_GUMBEL records (top_k = 0): the records already hold each 128 columns' winner
//   sample_nucleus_kernel       -- from f32 logits, with the exact selection of include/lrcn_nucleus.h in front of the draw: any top_k, top_p < 1
//                                  (lrcn_sample_batch_p where lrcn_sample_batch does not serve, and every lrcn_sample_logits call)
#include "kernels.h"

#include "common.h"
#include "gemm.h"
#include "draw.h"

namespace {

// row r takes token tok (log-probability lp) at step `current`; a finished row is frozen
__device__ __forceinline__ void sample_commit(const SampleState &s, int r, int tok, float lp) {
    if (s.done[r]) return;
    s.seq[(int64_t)r * s.L + s.current] = tok;
    s.last[r] = tok;
    s.logp[r] += lp;
    if (tok == s.eos || s.current > s.nword) {
        s.done[r] = 1;
        s.len[r] = s.current + 1;
        atomicAdd(s.ndone, 1);
    }
}

__global__ void sample_init_kernel(SampleState s, int R, int bos) {
    const int64_t n = (int64_t)R * s.L;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        s.seq[e] = (e % s.L) == 0 ? bos : 0;
        if (e < R) {
            s.last[e] = bos;
            s.logp[e] = 0.0f;
            s.done[e] = 0;
            s.len[e] = 0;
        }
    }
}

// One 256-thread workgroup per row of logits [R][ld]: max and sum exp in one pass over the row (staged in LDS up to V = 15360), the top_k
// boundary by top_k rounds of a block-wide argmax below the previous winner, then the Gumbel argmax over the admitted columns, four
// columns (one Philox call) per thread and round.
__global__ __launch_bounds__(256) void sample_rows_kernel(const float *logits, int64_t ld, int V, int top_k, float temp, uint32_t k0,
                                                          uint32_t k1, int S, int stage, SampleState s) {
    extern __shared__ float srow[];
    __shared__ float shf[4];
    __shared__ float shv[4];
    __shared__ int shi[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (s.done[r]) return;   // block-uniform
    const float *g = logits + (int64_t)r * ld;
    const float *z = stage ? srow : g;
    const float m = row_max_stage(g, V, stage, srow, shf);   // (its barriers also publish srow)
    float se = 0.0f;
    for (int j = tid; j < V; j += 256) se += __expf(z[j] - m);
    se = block_reduce(se, shf, false);
    const float lse = m + logf(se);
    // top_k boundary (tv, tc): column j is admitted iff (z_j, j) ranks no lower than it (larger z first, lower column in a tie)
    float tv = INFINITY;
    int tc = -1;
    for (int k = 0; k < top_k; ++k) {
        float bv = -INFINITY;
        int bi = 0x7FFFFFFF;
        for (int j = tid; j < V; j += 256) {
            const float x = z[j];
            if ((x < tv || (x == tv && j > tc)) && beats(x, j, bv, bi)) { bv = x; bi = j; }
        }
        block_best(bv, bi, shv, shi);
        tv = bv;
        tc = bi;
    }
    const float thr = temp > 0.0f ? m - GUMBEL_PRUNE * temp : m;
    const uint32_t si = (uint32_t)(r % S), ii = (uint32_t)(r / S);
    float bs, bz;
    int bc;
    gumbel_argmax(z, V, temp, thr, (uint32_t)s.current, si, ii, k0, k1,
                  [&](float x, int j) { return top_k == 0 || x > tv || (x == tv && j <= tc); }, bs, bc, bz);
    float wv = bs;
    int wc = bc;
    block_best(wv, wc, shv, shi);
    if (bc == wc && bs == wv) sample_commit(s, r, wc, bz - lse);   // exactly one thread holds the winning column
}

// Records of GEMM_OUT_SMAX_GUMBEL, one wave per row (4 rows per workgroup): lane l owns records l, l + 64, ...
template <int NR>
__global__ __launch_bounds__(256) void sample_gumbel_merge_kernel(const float *part, int nrec, int R, SampleState s) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R || s.done[row]) return;   // wave-uniform
    const float *rp = part + (int64_t)row * nrec * SMAX_REC;
    float m[NR], sx[NR];
    float bs = -INFINITY, bz = -INFINITY, gm = -INFINITY;
    int bc = 0x7FFFFFFF;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int rec = lane + 64 * q;
        m[q] = -INFINITY;
        sx[q] = 0.0f;
        if (rec < nrec) {
            const float4 a = *reinterpret_cast<const float4 *>(rp + (int64_t)rec * SMAX_REC);
            m[q] = a.x; sx[q] = a.y;
            const int c = __float_as_int(a.w);
            if (beats(a.z, c, bs, bc)) { bs = a.z; bc = c; bz = rp[(int64_t)rec * SMAX_REC + 4]; }
        }
        gm = fmaxf(gm, m[q]);
    }
    float se = 0.0f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gm = fmaxf(gm, __shfl_xor(gm, o));
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (m[q] != -INFINITY) se += sx[q] * __expf(m[q] - gm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    float wv = bs;
    int wc = bc;
    wave_best(wv, wc);
    const unsigned long long owner = __ballot(bc == wc && bs == wv);
    const float zt = __shfl(bz, (int)__ffsll((long long)owner) - 1);
    if (lane == 0) sample_commit(s, row, wc, zt - (gm + logf(se)));
}

// Records of GEMM_OUT_SMAX_TOPK (1 <= top_k < SMAX_KC), one wave per row: the row's top_k largest logits (ties by lower column) are the
// top_k best heads of the records' sorted lists -- exact, as a record keeps SMAX_KC > top_k of its columns -- and the draw is among them.
template <int NR>
__global__ __launch_bounds__(256) void sample_topk_merge_kernel(const float *part, int nrec, int R, int top_k, float temp, uint32_t k0, uint32_t k1,
                                                                int S, SampleState s) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R || s.done[row]) return;   // wave-uniform
    const float *rp = part + (int64_t)row * nrec * SMAX_REC;
    float m[NR], sx[NR], v[NR][SMAX_KC];
    int ix[NR][SMAX_KC];
    float gm = -INFINITY;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const int rec = lane + 64 * q;
        m[q] = -INFINITY;
        sx[q] = 0.0f;
#pragma unroll
        for (int j = 0; j < SMAX_KC; ++j) {
            v[q][j] = -INFINITY;
            ix[q][j] = 0x7FFFFFFF;
        }
        if (rec < nrec) {
            const float *p = rp + (int64_t)rec * SMAX_REC;
            m[q] = p[0]; sx[q] = p[1];
#pragma unroll
            for (int j = 0; j < SMAX_KC; ++j) {
                v[q][j] = p[2 + j];
                ix[q][j] = __float_as_int(p[8 + j]);
            }
        }
        gm = fmaxf(gm, m[q]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gm = fmaxf(gm, __shfl_xor(gm, o));
    float se = 0.0f;
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (m[q] != -INFINITY) se += sx[q] * __expf(m[q] - gm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    const float lse = gm + logf(se);
    const uint32_t si = (uint32_t)(row % S), ii = (uint32_t)(row / S);
    float bs = -INFINITY, bz = -INFINITY;
    int bc = 0x7FFFFFFF;
    for (int k = 0; k < top_k; ++k) {
        float lv = -INFINITY;
        int li = 0x7FFFFFFF;
#pragma unroll
        for (int q = 0; q < NR; ++q)
            if (beats(v[q][0], ix[q][0], lv, li)) { lv = v[q][0]; li = ix[q][0]; }
        float cv = lv;
        int ci = li;
        wave_best(cv, ci);   // the k-th largest logit of the row and its column (wave-uniform)
#pragma unroll
        for (int q = 0; q < NR; ++q)
            if (ix[q][0] == ci && v[q][0] == cv) {   // the owner retires it: shift the list (static indices only)
#pragma unroll
                for (int j = 0; j + 1 < SMAX_KC; ++j) {
                    v[q][j] = v[q][j + 1];
                    ix[q][j] = ix[q][j + 1];
                }
                v[q][SMAX_KC - 1] = -INFINITY;
                ix[q][SMAX_KC - 1] = 0x7FFFFFFF;
            }
        const float sc = temp > 0.0f ? cv / temp + gumbel_of(philox4x32_10((uint32_t)(ci >> 2), (uint32_t)s.current, si, ii, k0, k1).x[ci & 3]) : cv;
        if (beats(sc, ci, bs, bc)) { bs = sc; bc = ci; bz = cv; }
    }
    if (lane == 0) sample_commit(s, row, bc, bz - lse);
}

// ------------------------------------------------------------------------------------------- nucleus / any top_k (include/lrcn_nucleus.h)
// The order-preserving key of a float: a > b <=> okey(a) > okey(b), and -0 / +0 share one key (they are equal in the rank order).
__device__ __forceinline__ uint32_t okey(float x) {
    const uint32_t u = __float_as_uint(x == 0.0f ? 0.0f : x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int block_sum_int(int v, int *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// A prefix of the rank order: column j with key k belongs to it iff k > key, or k == key and j <= col.  {0, INT_MAX} is the whole row.
struct RankCut {
    uint32_t key;
    int col;
};
__device__ __forceinline__ bool in_cut(uint32_t k, int j, const RankCut &c) { return k > c.key || (k == c.key && j <= c.col); }

// The column of the need-th (1-based) column, in column order, whose key equals `key` (there are at least `need`).  Each thread counts a
// contiguous range of columns, a block-wide exclusive prefix count finds the range that holds it, and that range's thread walks to it.
__device__ int tie_column(const float *z, int V, uint32_t key, int need, int *shi, int *shcol) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int per = (V + 255) / 256, j0 = min(V, tid * per), j1 = min(V, j0 + per);
    int cnt = 0;
    for (int j = j0; j < j1; ++j) cnt += okey(z[j]) == key;
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) shi[w] = inc;
    __syncthreads();
    int before = inc - cnt;
    for (int q = 0; q < w; ++q) before += shi[q];
    if (before < need && need <= before + cnt) {   // exactly one thread
        int left = need - before, col = j0;
        for (int j = j0; j < j1; ++j)
            if (okey(z[j]) == key && --left == 0) { col = j; break; }
        *shcol = col;
    }
    __syncthreads();
    return *shcol;
}

struct NucleusArgs {
    const float *logits;
    int64_t ld;
    int V, top_k;
    float top_p, temp;
    uint32_t k0, k1;
    int S, current, stage;
    int32_t *count;       // row r's admitted-set size goes to count[r * count_ld] (NULL: not wanted)
    int64_t count_ld;
    int32_t *out_tok;     // without a SampleState (s.seq == NULL): token and log-probability of row r
    float *out_logp;
};

// One 256-thread workgroup per row, the row staged in LDS up to V = 15360 as in sample_rows_kernel.  The selection is bisection on the
// 32-bit key, most significant bit first: the largest key K with #{key_j >= K} >= top_k is the top_k boundary value (32 block-wide counts),
// the largest K with sum{w_j : j in A_k, key_j >= K} >= top_p * W the nucleus' (32 block-wide sums; w_j recomputed every round: there is no
// room for a second row).  Both conditions are monotone in K -- the f32 sum too, as its order is fixed and every rounding is monotone --
// so the bit-by-bit search finds them.  One more pass counts the columns above and at the boundary value; where only some of the tied
// columns are needed, tie_column picks them by column.  Every sum: per-thread partials in column order, then block_reduce's tree.
__global__ __launch_bounds__(256) void sample_nucleus_kernel(NucleusArgs a, SampleState s) {
    extern __shared__ float srow[];
    __shared__ float shf[4];
    __shared__ float shv[4];
    __shared__ int shi[4];
    __shared__ int shcol;
    const int r = blockIdx.x, tid = threadIdx.x, V = a.V;
    if (s.seq && s.done[r]) return;   // block-uniform
    const float *g = a.logits + (int64_t)r * a.ld;
    const float *z = a.stage ? srow : g;
    const float temp = a.temp;
    const float m = row_max_stage(g, V, a.stage, srow, shf);   // (its barriers also publish srow)
    float se = 0.0f;
    for (int j = tid; j < V; j += 256) se += __expf(z[j] - m);
    se = block_reduce(se, shf, false);
    const float lse = m + logf(se);

    RankCut cut{0u, 0x7FFFFFFF};
    int n = V;
    if (temp > 0.0f && a.top_k > 0 && a.top_k < V) {
        uint32_t K = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = K | (1u << bit);
            int c = 0;
            for (int j = tid; j < V; j += 256) c += okey(z[j]) >= cand;
            if (block_sum_int(c, shi) >= a.top_k) K = cand;
        }
        int cg = 0, ce = 0;
        for (int j = tid; j < V; j += 256) {
            const uint32_t k = okey(z[j]);
            cg += k > K;
            ce += k == K;
        }
        cg = block_sum_int(cg, shi);
        ce = block_sum_int(ce, shi);
        const int need = a.top_k - cg;   // 1 <= need <= ce
        cut.key = K;
        cut.col = need >= ce ? 0x7FFFFFFF : tie_column(z, V, K, need, shi, &shcol);
        n = a.top_k;
    }
    if (temp > 0.0f && a.top_p < 1.0f) {
        const float invT = 1.0f / temp;
        const RankCut ak = cut;
        float W = 0.0f;
        for (int j = tid; j < V; j += 256) {
            const float x = z[j];
            if (in_cut(okey(x), j, ak)) W += __expf((x - m) * invT);
        }
        W = block_reduce(W, shf, false);
        const float target = a.top_p * W;
        uint32_t K = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = K | (1u << bit);
            float sw = 0.0f;
            for (int j = tid; j < V; j += 256) {
                const float x = z[j];
                const uint32_t k = okey(x);
                if (k >= cand && in_cut(k, j, ak)) sw += __expf((x - m) * invT);
            }
            if (block_reduce(sw, shf, false) >= target) K = cand;
        }
        // K is the key of a column of A_k (the row's maximum satisfies the condition with its own key, and between two present keys the
        // sum does not change).  Above it: mass sg in cg columns; at it: ce columns of A_k, each of weight we
        float sg = 0.0f, we = 0.0f;
        int cg = 0, ce = 0;
        for (int j = tid; j < V; j += 256) {
            const float x = z[j];
            const uint32_t k = okey(x);
            if (!in_cut(k, j, ak)) continue;
            const float w = __expf((x - m) * invT);
            if (k > K) { sg += w; ++cg; }
            else if (k == K) { we = w; ++ce; }
        }
        sg = block_reduce(sg, shf, false);
        we = block_reduce(we, shf, true);
        cg = block_sum_int(cg, shi);
        ce = block_sum_int(ce, shi);
        // the smallest e >= 1 with sg + e * we >= target (block-uniform arithmetic), at most the ce there are
        int e = we > 0.0f ? (int)fminf(ceilf((target - sg) / we), (float)ce) : ce;
        e = max(1, min(e, ce));
        while (e > 1 && sg + (float)(e - 1) * we >= target) --e;
        while (e < ce && sg + (float)e * we < target) ++e;
        n = cg + e;
        if (e < ce) {
            cut.key = K;
            cut.col = tie_column(z, V, K, e, shi, &shcol);
        } else if (K != ak.key) {
            cut.key = K;
            cut.col = 0x7FFFFFFF;
        }   // else: all of A_k's columns at its own boundary value -- the nucleus is A_k
    }

    const float thr = temp > 0.0f ? m - GUMBEL_PRUNE * temp : m;
    const int current = s.seq ? s.current : a.current;
    const uint32_t si = (uint32_t)(r % a.S), ii = (uint32_t)(r / a.S);
    float bs, bz;
    int bc;
    gumbel_argmax(z, V, temp, thr, (uint32_t)current, si, ii, a.k0, a.k1, [&](float x, int j) { return in_cut(okey(x), j, cut); }, bs, bc, bz);
    float wv = bs;
    int wc = bc;
    block_best(wv, wc, shv, shi);
    if (bc == wc && bs == wv) {   // exactly one thread holds the winning column
        if (a.count) a.count[(int64_t)r * a.count_ld] = n;
        if (s.seq) {
            sample_commit(s, r, wc, bz - lse);
        } else {
            a.out_tok[r] = wc;
            if (a.out_logp) a.out_logp[r] = bz - lse;
        }
    }
}

}  // namespace

void k_sample_init(hipStream_t st, const SampleState &s, int R, int bos) {
    const int64_t n = (int64_t)R * s.L;
    hipLaunchKernelGGL(sample_init_kernel, dim3((unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256)), dim3(256), 0, st, s, R, bos);
}
void k_sample_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int top_k, float temp, uint64_t seed, int S, const SampleState &s) {
    const int stage = V <= 15360;   // 60 KB of LDS (+ the static few bytes: under the default 64 KB limit)
    hipLaunchKernelGGL(sample_rows_kernel, dim3(R), dim3(256), stage ? sizeof(float) * V : 0, st, logits, ld, V, top_k, temp, (uint32_t)seed,
                       (uint32_t)(seed >> 32), S, stage, s);
}
bool k_sample_gumbel_merge(hipStream_t st, const float *part, int nrec, int R, const SampleState &s) {
    const dim3 grid((R + 3) / 4);
    if (nrec <= 64) hipLaunchKernelGGL(sample_gumbel_merge_kernel<1>, grid, dim3(256), 0, st, part, nrec, R, s);
    else if (nrec <= 128) hipLaunchKernelGGL(sample_gumbel_merge_kernel<2>, grid, dim3(256), 0, st, part, nrec, R, s);
    else if (nrec <= 256) hipLaunchKernelGGL(sample_gumbel_merge_kernel<4>, grid, dim3(256), 0, st, part, nrec, R, s);
    else return false;
    return true;
}
bool k_sample_topk_merge(hipStream_t st, const float *part, int nrec, int R, int top_k, float temp, uint64_t seed, int S, const SampleState &s) {
    if (top_k < 1 || top_k >= SMAX_KC) return false;
    const dim3 grid((R + 3) / 4);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (nrec <= 64) hipLaunchKernelGGL(sample_topk_merge_kernel<1>, grid, dim3(256), 0, st, part, nrec, R, top_k, temp, k0, k1, S, s);
    else if (nrec <= 128) hipLaunchKernelGGL(sample_topk_merge_kernel<2>, grid, dim3(256), 0, st, part, nrec, R, top_k, temp, k0, k1, S, s);
    else if (nrec <= 256) hipLaunchKernelGGL(sample_topk_merge_kernel<4>, grid, dim3(256), 0, st, part, nrec, R, top_k, temp, k0, k1, S, s);
    else return false;
    return true;
}
void k_sample_nucleus(hipStream_t st, const float *logits, int64_t ld, int R, int V, int S, int current, float temp, int top_k, float top_p,
                      uint64_t seed, const SampleState *s, int32_t *count, int64_t count_ld, int32_t *out_tok, float *out_logp) {
    const int stage = V <= 15360;   // as k_sample_rows
    const NucleusArgs a{logits, ld, V, top_k, top_p, temp, (uint32_t)seed, (uint32_t)(seed >> 32), S, current, stage, count, count_ld, out_tok, out_logp};
    hipLaunchKernelGGL(sample_nucleus_kernel, dim3(R), dim3(256), stage ? sizeof(float) * V : 0, st, a, s ? *s : SampleState{});
}
