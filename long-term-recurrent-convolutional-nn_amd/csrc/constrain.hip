// constrain.hip -- the constrained top-K of a decode step (include/lrcn_constrain.h): the K best ALLOWED columns of every row of f32 logits,
// with the log-probabilities of the whole row (a ban removes a candidate, it does not renormalise).  It stands where softmax_topk_rows_kernel
// <Q, true> stands for the unconstrained n-best beam, between the step's logits and nbest.hip / diverse.hip, which see nothing but a
// different top-K.  One workgroup of 256 per row.  Behind it the same top-K for rows that know which forced words their history holds
// (include/lrcn_forced.h): the stay proposals, the move values and the state of every row, for forced.hip.
#include "kernel_util.h"

namespace {

constexpr int kMaxHist = 257;   // bos + LRCN_BEAM_MAXLEN - 2 words: every position a step may read

// The columns rule 3 of include/lrcn_constrain.h bans for a row whose history (bos first, `current` tokens) is in h: for every start i in
// [1, t - n + 1], t = current - 1, whose n-1 tokens equal the history's last n-1, the token behind them.  Calls ban(column) for each, from
// whichever thread finds it; a column outside [0, V) is never passed on (stale rows of dead beam slots hold anything).
template <class Ban> __device__ __forceinline__ void ngram_bans(const int32_t *h, int current, int n, int V, const Ban &ban) {
    const int t = current - 1;
    if (n < 1 || t < n - 1) return;
    for (int i = 1 + (int)threadIdx.x; i <= t - n + 1; i += blockDim.x) {
        bool same = true;
        for (int q = 0; q < n - 1; ++q) same &= h[i + q] == h[t - n + 2 + q];
        const int32_t w = h[i + n - 1];
        if (same && (unsigned)w < (unsigned)V) ban(w);
    }
}

// softmax_topk_rows_kernel<Q, true> (decode_kernels.hip) with a ban bitmap between its normaliser and its rounds.  max, sum and lse are
// that kernel's, instruction for instruction (__expf, the per-thread order, block_max / block_sum) over all V columns, banned ones included:
// with constraints that do not bind the two kernels return the same bits.  Then the row's bitmap is built in LDS -- the call's static
// bitmap, eos while current <= min_len, rule 3's columns from the history -- every thread retires its own banned columns, and the rounds,
// the 64-entry tie-group extension and the whole-row rescan run on what is left.  Every loop bound and break below is block-uniform.
template <int Q>
__global__ __launch_bounds__(256) void constrained_topk_rows_kernel(const float *logits, int64_t ld, int V, int K, ConstrainArgs a, int32_t *idx,
                                                                    float *val) {
    __shared__ float sh[8];
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float wv[64];
    __shared__ int wi[64];
    __shared__ uint32_t bm[Q * 32];   // (V + 31) / 32 <= 32 Q words
    __shared__ int32_t hs[kMaxHist];
    const int r = blockIdx.x;
    const float *row = logits + (int64_t)r * ld;  // ld % 4 == 0, 16-byte aligned rows: columns [V, ld) may be read, never used
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
    auto local_best = [&](float &lv, int &li) {
        lv = -INFINITY;
        li = 0x7FFFFFFF;
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x[q][j] > lv) {  // increasing index: strict > keeps the lowest index among equals
                    lv = x[q][j];
                    li = 4 * (threadIdx.x + 256 * q) + j;
                }
    };
    float lv;
    int li;
    local_best(lv, li);
    const float mx = block_max(lv, sh);
    float se = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) se += __expf(x[q][j] - mx);  // exp(-inf) = 0 for the padding
    se = block_sum(se, sh);
    // the row's bitmap
    const int nw = (V + 31) >> 5, cur = a.current;
    for (int w = threadIdx.x; w < nw; w += 256) bm[w] = a.ban ? a.ban[w] : 0u;
    for (int p = threadIdx.x; p < cur; p += 256) hs[p] = a.hist[(int64_t)r * a.ld_hist + p];   // cur <= kMaxHist (checked on the host)
    __syncthreads();
    if (threadIdx.x == 0 && cur <= a.min_len && (unsigned)a.eos < (unsigned)V) atomicOr(&bm[a.eos >> 5], 1u << (a.eos & 31));
    ngram_bans(hs, cur, a.ngram, V, [&](int w) { atomicOr(&bm[w >> 5], 1u << (w & 31)); });
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int v0 = 4 * (threadIdx.x + 256 * q);
        if (v0 < V) {   // one word holds the four columns (v0 % 4 == 0)
            const uint32_t bits = bm[v0 >> 5] >> (v0 & 31);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((bits >> j) & 1u) x[q][j] = -INFINITY;
        }
    }
    local_best(lv, li);
    // Rounds 0 .. K-1 take the K largest allowed logits; the rule ranks by float32 logp, and distinct logits can round to one logp, so the
    // rounds go on (at most to 64 entries) while the next candidate's logp equals the K-th winner's: the tie group's lowest columns win.
    float pK = 0.0f, prev_pv = 0.0f;
    int n = 0, run = 0, n_gt = 0;   // run: first round of the current equal-logp run; n_gt: winners above pK
    for (int k = 0; k < 64; ++k) {
        float bv = lv;
        int bi = li;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
            sv[threadIdx.x >> 6] = bv;
            si[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        bv = sv[0];
        bi = si[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) {
                bv = sv[w];
                bi = si[w];
            }
        const float pv = (bv - mx) - logf(se);
        if (k >= K && (pv != pK || bi == 0x7FFFFFFF)) break;  // uniform: every thread holds the same (bv, bi)
        if (threadIdx.x == 0) {
            wi[k] = bi;
            wv[k] = pv;
        }
        n = k + 1;
        if (k == 0 || pv != prev_pv) run = k;
        prev_pv = pv;
        if (k == K - 1) {
            pK = pv;
            n_gt = run;
        }
        if (((bi >> 2) & 255) == (int)threadIdx.x) {  // the owner retires the winner and finds its next candidate
            const int slot = bi >> 10, j0 = bi & 3;
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q == slot && j == j0) x[q][j] = -INFINITY;
            local_best(lv, li);
        }
    }
    // 64 rounds without a break: the tie group may go on beyond them, and an unvisited member may have a lower column than a visited one.
    // Then the group's share of the K is taken from the whole row: the n_gt winners above pK stay, and the K - n_gt lowest ALLOWED columns
    // whose logp is pK follow, one block-wide minimum per slot (softmax_topk_rows_kernel's rescan, with the bitmap).
    if (n == 64) {
        int prev = -1;
        for (int k = n_gt; k < K; ++k) {
            int bi = 0x7FFFFFFF;
            for (int v = threadIdx.x; v < V; v += 256) {  // this thread's lowest qualifying column
                if (v > prev && !((bm[v >> 5] >> (v & 31)) & 1u) && (row[v] - mx) - logf(se) == pK) {
                    bi = v;
                    break;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) bi = min(bi, __shfl_xor(bi, o));
            __syncthreads();
            if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = bi;
            __syncthreads();
            bi = min(min(si[0], si[1]), min(si[2], si[3]));
            if (threadIdx.x == 0) {
                wi[k] = bi;
                wv[k] = pK;
            }
            prev = bi;
        }
        n = K;
    }
    if (threadIdx.x == 0) {
        for (int k = 1; k < n; ++k) {  // equal logp (distinct logits, same float): ascending column
            const float v = wv[k];
            const int ix = wi[k];
            int q = k;
            while (q > 0 && wv[q - 1] == v && wi[q - 1] > ix) {
                wv[q] = wv[q - 1];
                wi[q] = wi[q - 1];
                --q;
            }
            wv[q] = v;
            wi[q] = ix;
        }
        // fewer than K finite allowed logits (the host's feasibility bound rules it out for finite rows): column 0 at -inf, never an index
        // that a later kernel could read through
        for (int k = 0; k < K; ++k) {
            const bool none = wi[k] == 0x7FFFFFFF;
            idx[(int64_t)r * K + k] = none ? 0 : wi[k];
            val[(int64_t)r * K + k] = none ? -INFINITY : wv[k];
        }
    }
}

// The general form's middle step, any V: -inf over the row's banned columns of lp [R][ld] (the row's log-softmax), by the same three rules,
// straight to memory -- no bitmap of the row is kept.  Several threads may write the same -inf to one column.
__global__ __launch_bounds__(256) void constrain_mask_rows_kernel(float *lp, int64_t ld, int V, ConstrainArgs a) {
    __shared__ int32_t hs[kMaxHist];
    const int r = blockIdx.x, cur = a.current;
    float *row = lp + (int64_t)r * ld;
    for (int p = threadIdx.x; p < cur; p += 256) hs[p] = a.hist[(int64_t)r * a.ld_hist + p];
    __syncthreads();
    if (a.ban)
        for (int v = threadIdx.x; v < V; v += 256)
            if ((a.ban[v >> 5] >> (v & 31)) & 1u) row[v] = -INFINITY;
    if (threadIdx.x == 0 && cur <= a.min_len && (unsigned)a.eos < (unsigned)V) row[a.eos] = -INFINITY;
    ngram_bans(hs, cur, a.ngram, V, [&](int w) { row[w] = -INFINITY; });
}

// ---------------------------------------------------------------------------------------------- forced words (include/lrcn_forced.h)
// The sets of the image's words fw [C*A] (-1: no word) that the history in h (bos first, `current` tokens) has met: every thread compares
// its positions with the at most 12 words and ORs what it finds into *mask (LDS).  A word is in [1, V), so a stale token outside [0, V)
// matches none.
__device__ __forceinline__ void forced_state(const int32_t *h, int current, const int32_t *fw, int CA, int A, uint32_t *mask) {
    for (int p = 1 + (int)threadIdx.x; p < current; p += blockDim.x) {
        const int32_t w = h[p];
        uint32_t m = 0;
        for (int q = 0; q < CA; ++q) m |= (fw[q] >= 0 && fw[q] == w) ? 1u << (q / A) : 0u;
        if (m) atomicOr(mask, m);
    }
}
__device__ __forceinline__ uint32_t forced_full(const int32_t *fw, int CA, int A) {   // the image's present sets
    uint32_t full = 0;
    for (int q = 0; q < CA; ++q) full |= fw[q] >= 0 ? 1u << (q / A) : 0u;
    return full;
}

// constrained_topk_rows_kernel<Q> for a row that knows its state.  The loads, max, sum and lse are that kernel's, instruction for
// instruction.  Between them and the rounds: the bitmap of rules 1-3 and the row's state (from its history in LDS, an atomic OR into one
// mask word) are built side by side; after that barrier thread c * A + a reads its word's logit from global memory -- the move value, or
// -inf if the word is absent, its set satisfied or its bit set -- and, one barrier on (every move thread has read the bitmap of rules
// 1-3), the words of the unsatisfied sets and rule 4's eos bit are ORed in.  After one more barrier the masking, the rounds, the tie-group
// extension and the rescan run unchanged: they yield the row's K best STAY columns.  x[q][j] is never indexed dynamically; every loop
// bound and barrier is block-uniform.
template <int Q>
__global__ __launch_bounds__(256) void forced_topk_rows_kernel(const float *logits, int64_t ld, int V, int K, ConstrainArgs a, ForcedArgs f,
                                                               int32_t *idx, float *val, float *move, int32_t *state) {
    __shared__ float sh[8];
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float wv[64];
    __shared__ int wi[64];
    __shared__ uint32_t bm[Q * 32];   // (V + 31) / 32 <= 32 Q words
    __shared__ int32_t hs[kMaxHist];
    __shared__ int32_t fw[kForcedMaxWords];
    __shared__ uint32_t smask;
    const int r = blockIdx.x;
    const float *row = logits + (int64_t)r * ld;  // ld % 4 == 0, 16-byte aligned rows: columns [V, ld) may be read, never used
    float x[Q][4];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int v0 = 4 * (threadIdx.x + 256 * q);
        float4 f4 = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (v0 < V) f4 = *reinterpret_cast<const float4 *>(row + v0);
        x[q][0] = f4.x;
        x[q][1] = v0 + 1 < V ? f4.y : -INFINITY;
        x[q][2] = v0 + 2 < V ? f4.z : -INFINITY;
        x[q][3] = v0 + 3 < V ? f4.w : -INFINITY;
    }
    auto local_best = [&](float &lv, int &li) {
        lv = -INFINITY;
        li = 0x7FFFFFFF;
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x[q][j] > lv) {  // increasing index: strict > keeps the lowest index among equals
                    lv = x[q][j];
                    li = 4 * (threadIdx.x + 256 * q) + j;
                }
    };
    float lv;
    int li;
    local_best(lv, li);
    const float mx = block_max(lv, sh);
    float se = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) se += __expf(x[q][j] - mx);  // exp(-inf) = 0 for the padding
    se = block_sum(se, sh);
    // the row's bitmap, history and words
    const int nw = (V + 31) >> 5, cur = a.current, CA = f.C * f.A;
    for (int w = threadIdx.x; w < nw; w += 256) bm[w] = a.ban ? a.ban[w] : 0u;
    for (int p = threadIdx.x; p < cur; p += 256) hs[p] = a.hist[(int64_t)r * a.ld_hist + p];   // cur <= kMaxHist (checked on the host)
    if ((int)threadIdx.x < CA) fw[threadIdx.x] = f.words[(int64_t)(r / f.rows_per_image) * CA + threadIdx.x];   // CA <= 12 (host)
    if (threadIdx.x == 0) smask = 0u;
    __syncthreads();
    if (threadIdx.x == 0 && cur <= a.min_len && (unsigned)a.eos < (unsigned)V) atomicOr(&bm[a.eos >> 5], 1u << (a.eos & 31));
    ngram_bans(hs, cur, a.ngram, V, [&](int w) { atomicOr(&bm[w >> 5], 1u << (w & 31)); });
    forced_state(hs, cur, fw, CA, f.A, &smask);
    __syncthreads();
    const uint32_t st = smask, full = forced_full(fw, CA, f.A);
    int32_t my = -1;   // this thread's move word, if its set is present and not yet met (a word is in [1, V): checked on the host)
    float mv = -INFINITY;
    if ((int)threadIdx.x < CA) {
        const int32_t w = fw[threadIdx.x];
        if (w >= 0 && !((st >> (threadIdx.x / f.A)) & 1u)) {
            my = w;
            if (!((bm[w >> 5] >> (w & 31)) & 1u)) mv = (row[w] - mx) - logf(se);
        }
    }
    __syncthreads();   // every move thread has read the bitmap of rules 1-3
    if (my >= 0) atomicOr(&bm[my >> 5], 1u << (my & 31));
    if (threadIdx.x == 0 && st != full && (unsigned)a.eos < (unsigned)V) atomicOr(&bm[a.eos >> 5], 1u << (a.eos & 31));   // rule 4
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int v0 = 4 * (threadIdx.x + 256 * q);
        if (v0 < V) {   // one word holds the four columns (v0 % 4 == 0)
            const uint32_t bits = bm[v0 >> 5] >> (v0 & 31);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((bits >> j) & 1u) x[q][j] = -INFINITY;
        }
    }
    local_best(lv, li);
    // the rounds, the tie-group extension and the rescan of constrained_topk_rows_kernel (see there)
    float pK = 0.0f, prev_pv = 0.0f;
    int n = 0, run = 0, n_gt = 0;   // run: first round of the current equal-logp run; n_gt: winners above pK
    for (int k = 0; k < 64; ++k) {
        float bv = lv;
        int bi = li;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) {
            sv[threadIdx.x >> 6] = bv;
            si[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        bv = sv[0];
        bi = si[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) {
                bv = sv[w];
                bi = si[w];
            }
        const float pv = (bv - mx) - logf(se);
        if (k >= K && (pv != pK || bi == 0x7FFFFFFF)) break;  // uniform: every thread holds the same (bv, bi)
        if (threadIdx.x == 0) {
            wi[k] = bi;
            wv[k] = pv;
        }
        n = k + 1;
        if (k == 0 || pv != prev_pv) run = k;
        prev_pv = pv;
        if (k == K - 1) {
            pK = pv;
            n_gt = run;
        }
        if (((bi >> 2) & 255) == (int)threadIdx.x) {  // the owner retires the winner and finds its next candidate
            const int slot = bi >> 10, j0 = bi & 3;
#pragma unroll
            for (int q = 0; q < Q; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q == slot && j == j0) x[q][j] = -INFINITY;
            local_best(lv, li);
        }
    }
    if (n == 64) {
        int prev = -1;
        for (int k = n_gt; k < K; ++k) {
            int bi = 0x7FFFFFFF;
            for (int v = threadIdx.x; v < V; v += 256) {  // this thread's lowest qualifying column
                if (v > prev && !((bm[v >> 5] >> (v & 31)) & 1u) && (row[v] - mx) - logf(se) == pK) {
                    bi = v;
                    break;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) bi = min(bi, __shfl_xor(bi, o));
            __syncthreads();
            if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = bi;
            __syncthreads();
            bi = min(min(si[0], si[1]), min(si[2], si[3]));
            if (threadIdx.x == 0) {
                wi[k] = bi;
                wv[k] = pK;
            }
            prev = bi;
        }
        n = K;
    }
    if ((int)threadIdx.x < CA) move[(int64_t)r * CA + threadIdx.x] = mv;
    if (threadIdx.x == 0) {
        state[r] = (int32_t)st;
        for (int k = 1; k < n; ++k) {  // equal logp (distinct logits, same float): ascending column
            const float v = wv[k];
            const int ix = wi[k];
            int q = k;
            while (q > 0 && wv[q - 1] == v && wi[q - 1] > ix) {
                wv[q] = wv[q - 1];
                wi[q] = wi[q - 1];
                --q;
            }
            wv[q] = v;
            wi[q] = ix;
        }
        // fewer than K finite stay columns (the host's feasibility bound rules it out for finite rows): column 0 at -inf
        for (int k = 0; k < K; ++k) {
            const bool none = wi[k] == 0x7FFFFFFF;
            idx[(int64_t)r * K + k] = none ? 0 : wi[k];
            val[(int64_t)r * K + k] = none ? -INFINITY : wv[k];
        }
    }
}

// The general form's middle step, any V: lp [R][ld] holds the rows' log-softmax.  The row's state and rule 3's verdict on its move words
// come from the history; the move values are read from lp (-inf by the rules above) BEFORE anything is written; then -inf goes over every
// column that is no stay column: rules 1-3, eos unless the row is accepting, the words of the unsatisfied sets.
__global__ __launch_bounds__(256) void forced_mask_rows_kernel(float *lp, int64_t ld, int V, ConstrainArgs a, ForcedArgs f, float *move,
                                                               int32_t *state) {
    __shared__ int32_t hs[kMaxHist];
    __shared__ int32_t fw[kForcedMaxWords];
    __shared__ uint32_t smask, sban;   // sets met; move words that rule 3 bans
    const int r = blockIdx.x, cur = a.current, CA = f.C * f.A;
    float *row = lp + (int64_t)r * ld;
    for (int p = threadIdx.x; p < cur; p += 256) hs[p] = a.hist[(int64_t)r * a.ld_hist + p];
    if ((int)threadIdx.x < CA) fw[threadIdx.x] = f.words[(int64_t)(r / f.rows_per_image) * CA + threadIdx.x];
    if (threadIdx.x == 0) smask = sban = 0u;
    __syncthreads();
    ngram_bans(hs, cur, a.ngram, V, [&](int w) {
        uint32_t m = 0;
        for (int q = 0; q < CA; ++q) m |= fw[q] == w ? 1u << q : 0u;
        if (m) atomicOr(&sban, m);
    });
    forced_state(hs, cur, fw, CA, f.A, &smask);
    __syncthreads();
    const uint32_t st = smask, full = forced_full(fw, CA, f.A);
    int32_t my = -1;
    float mv = -INFINITY;
    if ((int)threadIdx.x < CA) {
        const int32_t w = fw[threadIdx.x];
        if (w >= 0 && !((st >> (threadIdx.x / f.A)) & 1u)) {
            my = w;
            const bool banned = (a.ban && ((a.ban[w >> 5] >> (w & 31)) & 1u)) || ((sban >> threadIdx.x) & 1u);
            if (!banned) mv = row[w];
        }
    }
    __syncthreads();   // the move values are in registers
    if (a.ban)
        for (int v = threadIdx.x; v < V; v += 256)
            if ((a.ban[v >> 5] >> (v & 31)) & 1u) row[v] = -INFINITY;
    if (threadIdx.x == 0 && (cur <= a.min_len || st != full) && (unsigned)a.eos < (unsigned)V) row[a.eos] = -INFINITY;
    ngram_bans(hs, cur, a.ngram, V, [&](int w) { row[w] = -INFINITY; });
    if (my >= 0) row[my] = -INFINITY;
    if ((int)threadIdx.x < CA) move[(int64_t)r * CA + threadIdx.x] = mv;
    if (threadIdx.x == 0) state[r] = (int32_t)st;
}

}  // namespace

bool k_constrained_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, const ConstrainArgs &a, int32_t *idx,
                             float *val) {
    if (V > 16384 || K > 32 || (ld % 4) || (reinterpret_cast<uintptr_t>(logits) & 15) || a.current > kMaxHist) return false;
    const int q = (V + 1023) / 1024;
    if (q <= 4)
        hipLaunchKernelGGL((constrained_topk_rows_kernel<4>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, idx, val);
    else if (q <= 8)
        hipLaunchKernelGGL((constrained_topk_rows_kernel<8>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, idx, val);
    else if (q <= 12)
        hipLaunchKernelGGL((constrained_topk_rows_kernel<12>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, idx, val);
    else
        hipLaunchKernelGGL((constrained_topk_rows_kernel<16>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, idx, val);
    return true;
}
void k_constrain_mask_rows(hipStream_t st, float *lp, int64_t ld, int R, int V, const ConstrainArgs &a) {
    hipLaunchKernelGGL(constrain_mask_rows_kernel, dim3(R), dim3(256), 0, st, lp, ld, V, a);
}

static_assert(kForcedMaxWords <= 32, "one bit per move word in forced_mask_rows_kernel's sban");
bool k_forced_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, const ConstrainArgs &a, const ForcedArgs &f,
                        int32_t *idx, float *val, float *move, int32_t *state) {
    if (V > 16384 || K > 32 || (ld % 4) || (reinterpret_cast<uintptr_t>(logits) & 15) || a.current > kMaxHist) return false;
    const int q = (V + 1023) / 1024;
    if (q <= 4)
        hipLaunchKernelGGL((forced_topk_rows_kernel<4>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, f, idx, val, move, state);
    else if (q <= 8)
        hipLaunchKernelGGL((forced_topk_rows_kernel<8>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, f, idx, val, move, state);
    else if (q <= 12)
        hipLaunchKernelGGL((forced_topk_rows_kernel<12>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, f, idx, val, move, state);
    else
        hipLaunchKernelGGL((forced_topk_rows_kernel<16>), dim3(R), dim3(256), 0, st, logits, ld, V, K, a, f, idx, val, move, state);
    return true;
}
void k_forced_mask_rows(hipStream_t st, float *lp, int64_t ld, int R, int V, const ConstrainArgs &a, const ForcedArgs &f, float *move,
                        int32_t *state) {
    hipLaunchKernelGGL(forced_mask_rows_kernel, dim3(R), dim3(256), 0, st, lp, ld, V, a, f, move, state);
}
