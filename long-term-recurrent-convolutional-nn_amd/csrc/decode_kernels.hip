// decode_kernels.hip -- the kernels only the caption decode (decode.hip) launches: beam initialisation and bookkeeping, top-K, softmax
// and log-softmax rows, their fused and records-merge forms, the parents' state gathers and the per-step operand preparation.
#include "kernel_util.h"

namespace {

__global__ void beam_init_kernel(int32_t *seq, int32_t *last, float *p, int R, int Lh, int bos) {
    const int64_t total = (int64_t)R * Lh;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i / Lh), j = (int)(i - (int64_t)q * Lh);
        seq[i] = j == 0 ? bos : 0;
        if (j == 0) {
            last[q] = bos;
            p[q] = 1.0f;
        }
    }
}

// Beam bookkeeping of ONE decode step for N images at once (lrcn.jl:657-677 per image), one workgroup per image:
//   candidates (i, j) = hypothesis i of the image x its j-th best next word, probability topv * p[i] (linear float32 space);
//   step 1 expands hypothesis 1 only (:662-664); stable descending order (ties: lower candidate index); keep K; stop when
//   the best ends in eos or current > nword (:670) -> the image is frozen and its result recorded.
// seq_in/seq_out: [N*K][L] token histories (ping-pong), p: [N*K] in/out, parent[N*K]: state row to copy, last[N*K]: token fed next.
__global__ __launch_bounds__(256) void beam_update_kernel(const int32_t *topi, const float *topv, const int32_t *seq_in, int32_t *seq_out,
                                                          float *p, int32_t *parent, int32_t *last, int32_t *done, int32_t *ndone,
                                                          int32_t *res_tok, int32_t *res_len, float *res_p, int K, int L, int current,
                                                          int nword, int eos) {
    __shared__ float cp[1024];
    __shared__ float newp[32];
    __shared__ int sel[32];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int r0 = n * K;
    if (done[n]) {  // frozen: identity parent, histories carried over
        for (int k = tid; k < K; k += blockDim.x) {
            parent[r0 + k] = r0 + k;
            last[r0 + k] = eos;
        }
        for (int e = tid; e < K * L; e += blockDim.x) seq_out[(int64_t)r0 * L + e] = seq_in[(int64_t)r0 * L + e];
        return;
    }
    const int nexp = current == 1 ? 1 : K, C = nexp * K;
    for (int c = tid; c < C; c += blockDim.x) cp[c] = topv[(int64_t)(r0 + c / K) * K + c % K] * p[r0 + c / K];
    __syncthreads();
    for (int c = tid; c < C; c += blockDim.x) {
        const float v = cp[c];
        int rank = 0;
        for (int q = 0; q < C; ++q) rank += (cp[q] > v) || (cp[q] == v && q < c);
        if (rank < K) {
            sel[rank] = c;
            newp[rank] = v;
        }
    }
    __syncthreads();
    // K <= C always (C >= K): every rank 0..K-1 is filled.  New histories = parent's history + the chosen word.
    for (int e = tid; e < K * L; e += blockDim.x) {
        const int k = e / L, pos = e - k * L;
        const int c = sel[k], i = c / K;
        int32_t t = seq_in[(int64_t)(r0 + i) * L + pos];
        if (pos == current) t = topi[(int64_t)(r0 + i) * K + c % K];
        seq_out[(int64_t)(r0 + k) * L + pos] = t;
    }
    __syncthreads();
    for (int k = tid; k < K; k += blockDim.x) {
        const int c = sel[k];
        p[r0 + k] = newp[k];
        parent[r0 + k] = r0 + c / K;
        last[r0 + k] = topi[(int64_t)(r0 + c / K) * K + c % K];
    }
    if (tid == 0) {
        const int c = sel[0];
        const int best_tok = topi[(int64_t)(r0 + c / K) * K + c % K];
        if (best_tok == eos || current > nword) {
            done[n] = 1;
            atomicAdd(ndone, 1);
            res_len[n] = current + 1;
            res_p[n] = newp[0];
        }
    }
    __syncthreads();
    if (done[n])
        for (int pos = tid; pos <= current; pos += blockDim.x) res_tok[(int64_t)n * L + pos] = seq_out[(int64_t)r0 * L + pos];
}
// out[r][0..C) = in[r / K][0..C)  (replicate each image row K times)
template <typename T> __global__ void repeat_rows_kernel(const T *in, int64_t ld, int R, int K, int C, T *out) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) out[(int64_t)r * ld + c] = in[(int64_t)(r / K) * ld + c];
}

__global__ __launch_bounds__(256) void softmax_rows_kernel(const float *logits, int64_t ld_l, int M, int V, float *prob,
                                                           int64_t ld_p) {
    __shared__ float sh[8];
    const int m = blockIdx.x;
    const float *row = logits + (int64_t)m * ld_l;
    float mx = -INFINITY;
    for (int v = threadIdx.x; v < V; v += blockDim.x) mx = fmaxf(mx, row[v]);
    mx = block_max(mx, sh);
    float se = 0.0f;
    for (int v = threadIdx.x; v < V; v += blockDim.x) se += expf(row[v] - mx);
    se = block_sum(se, sh);
    const float lse = mx + logf(se);
    for (int v = threadIdx.x; v < V; v += blockDim.x) prob[(int64_t)m * ld_p + v] = expf(row[v] - lse);
}

// log softmax of each row, (x - max) - log(sum exp(x - max)): the n-best beam's fallback above softmax_topk_rows_kernel's V limit
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float *logits, int64_t ld_l, int M, int V, float *out, int64_t ld_o) {
    __shared__ float sh[8];
    const int m = blockIdx.x;
    const float *row = logits + (int64_t)m * ld_l;
    float mx = -INFINITY;
    for (int v = threadIdx.x; v < V; v += blockDim.x) mx = fmaxf(mx, row[v]);
    mx = block_max(mx, sh);
    float se = 0.0f;
    for (int v = threadIdx.x; v < V; v += blockDim.x) se += expf(row[v] - mx);
    se = block_sum(se, sh);
    const float ls = logf(se);
    for (int v = threadIdx.x; v < V; v += blockDim.x) out[(int64_t)m * ld_o + v] = (row[v] - mx) - ls;
}

// Top-K of each row, descending, ties to the lower index (Julia's stable sortperm(rev=true), lrcn.jl:655).
// One 256-thread block per row; K rounds of block-wide argmax with the winners masked out. K <= 32.
__global__ __launch_bounds__(256) void topk_rows_kernel(const float *prob, int64_t ld, int R, int V, int K, int32_t *idx,
                                                        float *val) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int chosen[32];
    const int r = blockIdx.x;
    const float *row = prob + (int64_t)r * ld;
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = 0x7FFFFFFF;
        for (int v = threadIdx.x; v < V; v += blockDim.x) {
            bool taken = false;
            for (int q = 0; q < k; ++q) taken |= (chosen[q] == v);
            const float x = row[v];
            if (!taken && (x > bv || (x == bv && v < bi))) {
                bv = x;
                bi = v;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((threadIdx.x & 63) == 0) {
            sv[threadIdx.x >> 6] = bv;
            si[threadIdx.x >> 6] = bi;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w)
                if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) {
                    bv = sv[w];
                    bi = si[w];
                }
            chosen[k] = bi;
            idx[r * K + k] = bi;
            val[r * K + k] = bv;
        }
        __syncthreads();
    }
}

// softmax_rows + topk_rows in one pass for V <= 16384: the row of logits stays in registers; the K winners are the K largest
// LOGITS (softmax is monotone; ties to the lower index), their probabilities expf(x - (max + logf(sum))) are computed for
// those K only, and winners whose float probabilities coincide are put in ascending index order, which is the order
// topk_rows_kernel (Julia's stable sortperm(rev=true), lrcn.jl:655) gives on the probabilities.  The normaliser uses the
// hardware exponential (one instruction per element instead of ~20): 1e-6 relative on the reported probabilities.
// Q = float4 loads per thread: V <= 1024 Q.  Every thread keeps the best of its own not-yet-retired elements; a round is
// one block-wide argmax over those 256 candidates, after which only the winner's owner rescans its registers.
// LOGP (the n-best beam, lrcn_nbest.h): the values are log-probabilities (x - max) - log(sum) instead, computed from the logit and
// not as log(p) (p underflows to 0 for the improbable words of a peaked row); the same ranking and tie-group rule on those values.
template <int Q, bool LOGP = false>
__global__ __launch_bounds__(256) void softmax_topk_rows_kernel(const float *logits, int64_t ld, int R, int V, int K, int32_t *idx,
                                                                float *val) {
    __shared__ float sh[8];
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float wv[64];
    __shared__ int wi[64];
    const int r = blockIdx.x;
    const float *row = logits + (int64_t)r * ld;  // ld % 4 == 0, 16-byte aligned rows: columns [V, ld) may be read, never used
    float x[Q][4];
    // thread t owns columns 4 (t + 256 q) .. + 3
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
    const float lse = mx + logf(se);
    // Rounds 0 .. K-1 take the K largest logits.  The reference ranks the float32 PROBABILITIES with a stable sort (lrcn.jl:652-656),
    // and distinct logits can round to one float probability: if candidates beyond the K-th still share the K-th winner's
    // probability they belong to the same tie group, whose lowest INDICES win.  So the rounds go on (at most to 64 entries)
    // until the next candidate's probability differs; all of this is block-uniform.
    float pK = -1.0f, prev_pv = 0.0f;
    int n = 0, run = 0, n_gt = 0;   // run: first round of the current equal-probability run; n_gt: winners above pK
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
        const float pv = LOGP ? (bv - mx) - logf(se) : expf(bv - lse);
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
    // 64 rounds without a break: the tie group may go on beyond them (more distinct logits within one float probability than the rounds
    // visit, in descending LOGIT order), and an unvisited member may have a lower index than a visited one.  Then the group's share of the
    // K is taken from the whole row instead: the n_gt winners above pK stay, and the K - n_gt lowest columns whose probability is pK follow,
    // one block-wide minimum per slot.  (Block-uniform; a flat model with > 64 logits inside one float probability gets here.  A group that
    // ends exactly at round 63 also does, harmlessly: the rescan returns the same columns.)
    if (n == 64) {
        int prev = -1;
        for (int k = n_gt; k < K; ++k) {
            int bi = 0x7FFFFFFF;
            for (int v = threadIdx.x; v < V; v += 256) {  // this thread's lowest qualifying column
                const float xv = row[v];
                if (v > prev && (LOGP ? (xv - mx) - logf(se) : expf(xv - lse)) == pK) {
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
        for (int k = 1; k < n; ++k) {  // equal probabilities (distinct logits, same float): ascending index
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
        for (int k = 0; k < K; ++k) {
            idx[r * K + k] = wi[k];
            val[r * K + k] = wv[k];
        }
    }
}

// The second half of GEMM_OUT_SMAX_TOPK (gemm.h SmaxEpi; round 6): one wave per row combines the row's nrec = V / 128 records {max, sum exp,
// SMAX_KC best logits + columns} into what softmax_topk_rows_kernel returns for the full row of logits: the K largest float32
// PROBABILITIES p = exp(x - lse), lse = max + log(sum), in descending order, equal probabilities by ascending column (lrcn.jl:652-656 --
// a stable descending sort of p).  As there, the rounds go on past K while the next candidate still shares the K-th probability
// (distinct logits that round to one float), then the tie group is put in index order.  A record keeps SMAX_KC = K + 1 candidates
// of its 128 columns, so a tie group that crosses the K boundary is exact as long as no more than SMAX_KC of it fall into one record.
// Lane l owns records l, l + 64, ...; every record's list is sorted, so a lane's best candidate is the best list HEAD, and retiring a
// candidate shifts that list (static indices only).  LOGP: log-probabilities (x - max) - log(sum), as softmax_topk_rows_kernel<Q, true>.
template <int NR, bool LOGP = false>
__global__ __launch_bounds__(256) void softmax_topk_merge_kernel(const float *part, int nrec, int R, int K, int32_t *idx, float *val) {
    __shared__ float wv[4][64];
    __shared__ int wi[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + w;
    if (row >= R) return;   // wave-uniform; no block-wide barrier below
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
            const float4 a = *reinterpret_cast<const float4 *>(rp + (int64_t)rec * SMAX_REC), b = *reinterpret_cast<const float4 *>(rp + (int64_t)rec * SMAX_REC + 4),
                         c = *reinterpret_cast<const float4 *>(rp + (int64_t)rec * SMAX_REC + 8), d = *reinterpret_cast<const float4 *>(rp + (int64_t)rec * SMAX_REC + 12);
            m[q] = a.x; sx[q] = a.y;
            v[q][0] = a.z; v[q][1] = a.w; v[q][2] = b.x; v[q][3] = b.y; v[q][4] = b.z; v[q][5] = b.w;
            ix[q][0] = __float_as_int(c.x); ix[q][1] = __float_as_int(c.y); ix[q][2] = __float_as_int(c.z); ix[q][3] = __float_as_int(c.w);
            ix[q][4] = __float_as_int(d.x); ix[q][5] = __float_as_int(d.y);
        }
        gm = fmaxf(gm, m[q]);
    }
    gm = wave_max(gm);
    float se = 0.0f;
#pragma unroll
    for (int q = 0; q < NR; ++q)
        if (m[q] != -INFINITY) se += sx[q] * __expf(m[q] - gm);
    se = wave_sum(se);
    const float lse = gm + logf(se);
    auto local_best = [&](float &lv, int &li) {
        lv = -INFINITY;
        li = 0x7FFFFFFF;
#pragma unroll
        for (int q = 0; q < NR; ++q)
            if (v[q][0] > lv || (v[q][0] == lv && ix[q][0] < li)) {
                lv = v[q][0];
                li = ix[q][0];
            }
    };
    float lv;
    int li;
    local_best(lv, li);
    float pK = -1.0f;
    int n = 0;
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
        const float pv = LOGP ? (bv - gm) - logf(se) : expf(bv - lse);
        if (k >= K && (pv != pK || bi == 0x7FFFFFFF)) break;  // wave-uniform
        if (lane == 0) {
            wi[w][k] = bi;
            wv[w][k] = pv;
        }
        n = k + 1;
        if (k == K - 1) pK = pv;
        if (li == bi && bi != 0x7FFFFFFF) {  // the owner retires the winner: its list moves up by one
#pragma unroll
            for (int q = 0; q < NR; ++q)
                if (ix[q][0] == bi) {
#pragma unroll
                    for (int j = 0; j + 1 < SMAX_KC; ++j) {
                        v[q][j] = v[q][j + 1];
                        ix[q][j] = ix[q][j + 1];
                    }
                    v[q][SMAX_KC - 1] = -INFINITY;
                    ix[q][SMAX_KC - 1] = 0x7FFFFFFF;
                }
            local_best(lv, li);
        }
    }
    if (lane == 0) {
        for (int k = 1; k < n; ++k) {  // equal probabilities (distinct logits, same float): ascending index
            const float vv = wv[w][k];
            const int ii = wi[w][k];
            int q = k;
            while (q > 0 && wv[w][q - 1] == vv && wi[w][q - 1] > ii) {
                wv[w][q] = wv[w][q - 1];
                wi[w][q] = wi[w][q - 1];
                --q;
            }
            wv[w][q] = vv;
            wi[w][q] = ii;
        }
        for (int k = 0; k < K; ++k) {
            idx[row * K + k] = wi[w][k];
            val[row * K + k] = wv[w][k];
        }
    }
}

// Beam reordering of the four recurrent state tensors in one launch (lrcn.jl:673-676): out[i][r] = in[i][parent[r]], plus
// the K-contiguous T copies of h1 / h2 that the next step's recurrent GEMMs read.
struct GatherState {
    const float *in[4];
    float *out[4];
    void *hT[4];     // T copy of state i (or NULL)
    int64_t ldT[4];
    int C[4];
};
template <typename T> __global__ void gather_state_kernel(const GatherState g, const int32_t *parent) {
    const int r = blockIdx.x, i = blockIdx.y;
    const int C = g.C[i];
    const float *s = g.in[i] + (int64_t)parent[r] * C;
    float *o = g.out[i] + (int64_t)r * C;
    T *t = g.hT[i] ? reinterpret_cast<T *>(g.hT[i]) + (int64_t)r * g.ldT[i] : nullptr;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float v = s[c];
        o[c] = v;
        if (t) t[c] = from_f32<T>(v);
    }
}

// The batched beam decode's per-step gather (round 6), bf16 only: row r of the next step's [x | h1] operand = the embedding of hypothesis
// r's last token (lrcn.jl:650) next to h1 of its PARENT hypothesis (lrcn.jl:673-676), and the h2 block of [x2 | h2] likewise -- what
// embed_gather + gather_state did in two launches, without the four f32 state tensors' round trip (82 MB in, 82 MB out per step at 5120
// hypotheses: the cell state now stays where the epilogue wrote it and is READ through `parent`, LstmEpi::c_prev_idx).  16-byte vectors:
// every row starts 128-byte aligned (leading dimensions are multiples of 64 elements).  parent == NULL: the first step (h blocks zero).
__global__ __launch_bounds__(256) void decode_prep_kernel(const bf16_t *wembT, int64_t ld_w, const int32_t *last, const int32_t *parent, int E,
                                                          const bf16_t *h1, int64_t ld_h1, int H1, const bf16_t *h2, int64_t ld_h2, int H2,
                                                          bf16_t *xh1, int64_t ld_xh1, int64_t off_h1, bf16_t *xh2, int64_t ld_xh2, int64_t off_h2) {
    const int r = blockIdx.x;
    auto copy = [&](const bf16_t *src, bf16_t *dst, int n) {   // exactly n elements: whole 16-byte vectors, then a scalar tail (LRCN-1f keeps
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);  // x_cnn right behind the embedding columns)
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int i = threadIdx.x; i < n / 8; i += 256) d4[i] = s4[i];
        for (int i = (n & ~7) + threadIdx.x; i < n; i += 256) dst[i] = src[i];
    };
    copy(wembT + (int64_t)last[r] * ld_w, xh1 + (int64_t)r * ld_xh1, E);
    if (parent) {
        const int pr = parent[r];
        copy(h1 + (int64_t)pr * ld_h1, xh1 + (int64_t)r * ld_xh1 + off_h1, H1);
        if (h2) copy(h2 + (int64_t)pr * ld_h2, xh2 + (int64_t)r * ld_xh2 + off_h2, H2);
    }
}

// The prep launch of the decode step with input-projection TABLES (decode.hip decode_tables; round 6): the gate GEMMs contract the hidden
// state alone, so only the parents' h move -- h1[parent] into the rows of A1, h2[parent] into the h block of A2 = [h1 Wproj | h2].
__global__ __launch_bounds__(256) void decode_prep_h_kernel(const int32_t *parent, const bf16_t *h1, int64_t ld_h1, int H1, const bf16_t *h2,
                                                            int64_t ld_h2, int H2, bf16_t *a1, int64_t ld_a1, bf16_t *a2, int64_t ld_a2, int64_t off_h2) {
    const int r = blockIdx.x, pr = parent[r];
    auto copy = [&](const bf16_t *src, bf16_t *dst, int n) {
        const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int i = threadIdx.x; i < n / 8; i += 256) d4[i] = s4[i];
        for (int i = (n & ~7) + threadIdx.x; i < n; i += 256) dst[i] = src[i];
    };
    copy(h1 + (int64_t)pr * ld_h1, a1 + (int64_t)r * ld_a1, H1);
    copy(h2 + (int64_t)pr * ld_h2, a2 + (int64_t)r * ld_a2 + off_h2, H2);
}
__global__ void row_div_kernel(int32_t *out, int R, int K) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < R) out[r] = r / K;
}

__global__ void gather_rows_f32_kernel(const float *in, int64_t ld, const int32_t *src_row, int R, int C, float *out) {
    const int r = blockIdx.x;
    const float *s = in + (int64_t)src_row[r] * ld;
    for (int c = threadIdx.x; c < C; c += blockDim.x) out[(int64_t)r * ld + c] = s[c];
}

}  // namespace
// ---------------------------------------------------------------- launchers
void k_beam_init(hipStream_t st, int32_t *seq, int32_t *last, float *p, int R, int Lh, int bos) {
    hipLaunchKernelGGL(beam_init_kernel, dim3(grid1d((int64_t)R * Lh)), dim3(256), 0, st, seq, last, p, R, Lh, bos);
}
void k_topk_rows(hipStream_t st, const float *prob, int64_t ld, int R, int V, int K, int32_t *idx, float *val) {
    hipLaunchKernelGGL(topk_rows_kernel, dim3(R), dim3(256), 0, st, prob, ld, R, V, K, idx, val);
}
void k_beam_update(hipStream_t st, const int32_t *topi, const float *topv, const int32_t *seq_in, int32_t *seq_out, float *p,
                   int32_t *parent, int32_t *last, int32_t *done, int32_t *ndone, int32_t *res_tok, int32_t *res_len, float *res_p, int N,
                   int K, int L, int current, int nword, int eos) {
    hipLaunchKernelGGL(beam_update_kernel, dim3(N), dim3(256), 0, st, topi, topv, seq_in, seq_out, p, parent, last, done, ndone, res_tok,
                       res_len, res_p, K, L, current, nword, eos);
}
void k_repeat_rows(hipStream_t st, int dtype, const void *in, int64_t ld, int N, int K, int C, void *out) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(repeat_rows_kernel<T>, dim3(N * K), dim3(256), 0, st, (const T *)in, ld, N * K, K, C, (T *)out));
}
void k_softmax_rows(hipStream_t st, const float *logits, int64_t ld_l, int M, int V, float *prob, int64_t ld_p) {
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(M), dim3(256), 0, st, logits, ld_l, M, V, prob, ld_p);
}
void k_log_softmax_rows(hipStream_t st, const float *logits, int64_t ld_l, int M, int V, float *out, int64_t ld_o) {
    hipLaunchKernelGGL(log_softmax_rows_kernel, dim3(M), dim3(256), 0, st, logits, ld_l, M, V, out, ld_o);
}
template <bool LOGP> void launch_softmax_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, int32_t *idx, float *val) {
    const int q = (V + 1023) / 1024;
    if (q <= 4)
        hipLaunchKernelGGL((softmax_topk_rows_kernel<4, LOGP>), dim3(R), dim3(256), 0, st, logits, ld, R, V, K, idx, val);
    else if (q <= 8)
        hipLaunchKernelGGL((softmax_topk_rows_kernel<8, LOGP>), dim3(R), dim3(256), 0, st, logits, ld, R, V, K, idx, val);
    else if (q <= 12)
        hipLaunchKernelGGL((softmax_topk_rows_kernel<12, LOGP>), dim3(R), dim3(256), 0, st, logits, ld, R, V, K, idx, val);
    else
        hipLaunchKernelGGL((softmax_topk_rows_kernel<16, LOGP>), dim3(R), dim3(256), 0, st, logits, ld, R, V, K, idx, val);
}
bool k_softmax_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, int32_t *idx, float *val, bool logp) {
    if (V > 16384 || K > 32 || (ld % 4) || (reinterpret_cast<uintptr_t>(logits) & 15)) return false;
    if (logp) launch_softmax_topk_rows<true>(st, logits, ld, R, V, K, idx, val);
    else launch_softmax_topk_rows<false>(st, logits, ld, R, V, K, idx, val);
    return true;
}
void k_gather_state(hipStream_t st, int dtype, const float *const in[4], float *const out[4], void *const hT[4], const int64_t ldT[4],
                    const int C[4], const int32_t *parent, int R) {
    GatherState g;
    for (int i = 0; i < 4; ++i) {
        g.in[i] = in[i]; g.out[i] = out[i]; g.hT[i] = hT[i]; g.ldT[i] = ldT[i]; g.C[i] = C[i];
    }
    DISPATCH_T(dtype, hipLaunchKernelGGL(gather_state_kernel<T>, dim3(R, 4), dim3(256), 0, st, g, parent));
}
template <bool LOGP> void launch_softmax_topk_merge(hipStream_t st, const float *part, int nrec, int R, int K, int32_t *idx, float *val) {
    const dim3 grid((R + 3) / 4);
    if (nrec <= 64) hipLaunchKernelGGL((softmax_topk_merge_kernel<1, LOGP>), grid, dim3(256), 0, st, part, nrec, R, K, idx, val);
    else if (nrec <= 128) hipLaunchKernelGGL((softmax_topk_merge_kernel<2, LOGP>), grid, dim3(256), 0, st, part, nrec, R, K, idx, val);
    else hipLaunchKernelGGL((softmax_topk_merge_kernel<4, LOGP>), grid, dim3(256), 0, st, part, nrec, R, K, idx, val);
}
bool k_softmax_topk_merge(hipStream_t st, const float *part, int nrec, int R, int K, int32_t *idx, float *val, bool logp) {
    if (K < 1 || K >= SMAX_KC || nrec < 1 || nrec > 256 || (reinterpret_cast<uintptr_t>(part) & 15)) return false;
    if (logp) launch_softmax_topk_merge<true>(st, part, nrec, R, K, idx, val);
    else launch_softmax_topk_merge<false>(st, part, nrec, R, K, idx, val);
    return true;
}
void k_decode_prep(hipStream_t st, const void *wembT, int64_t ld_w, const int32_t *last, const int32_t *parent, int R, int E, const void *h1,
                   int64_t ld_h1, int H1, const void *h2, int64_t ld_h2, int H2, void *xh1, int64_t ld_xh1, int64_t off_h1, void *xh2, int64_t ld_xh2,
                   int64_t off_h2) {
    hipLaunchKernelGGL(decode_prep_kernel, dim3(R), dim3(256), 0, st, (const bf16_t *)wembT, ld_w, last, parent, E, (const bf16_t *)h1, ld_h1, H1,
                       (const bf16_t *)h2, ld_h2, H2, (bf16_t *)xh1, ld_xh1, off_h1, (bf16_t *)xh2, ld_xh2, off_h2);
}
void k_decode_prep_h(hipStream_t st, const int32_t *parent, int R, const void *h1, int64_t ld_h1, int H1, const void *h2, int64_t ld_h2, int H2,
                     void *a1, int64_t ld_a1, void *a2, int64_t ld_a2, int64_t off_h2) {
    hipLaunchKernelGGL(decode_prep_h_kernel, dim3(R), dim3(256), 0, st, parent, (const bf16_t *)h1, ld_h1, H1, (const bf16_t *)h2, ld_h2, H2,
                       (bf16_t *)a1, ld_a1, (bf16_t *)a2, ld_a2, off_h2);
}
void k_row_div(hipStream_t st, int32_t *out, int R, int K) {
    hipLaunchKernelGGL(row_div_kernel, dim3((R + 255) / 256), dim3(256), 0, st, out, R, K);
}
void k_gather_rows_f32(hipStream_t st, const float *in, int64_t ld, const int32_t *src_row, int R, int C, float *out) {
    hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(R), dim3(256), 0, st, in, ld, src_row, R, C, out);
}
