// nbest.hip -- the per-step bookkeeping of the n-best beam search (lrcn_beam_nbest_batch, include/lrcn_nbest.h): log space, a pool of
// finished hypotheses per image, length normalisation and an exact early stop.  One workgroup per image, as beam_update_kernel; the
// step's log-probability top-K (softmax_topk_rows_kernel / softmax_topk_merge_kernel with LOGP) comes in topi / topv.
#include "kernels.h"

#include "common.h"
#include "nbest_pool.h"

namespace {

constexpr int kMaxK = 32;

__global__ void nbest_init_kernel(NbestState s, int N, int bos) {
    const int R = N * s.K;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
        const_cast<int32_t *>(s.seq_in)[(int64_t)r * s.L] = bos;
        s.last[r] = bos;
        s.parent[r] = r;
        s.cum[r] = 0.0f;
        if (r < N) s.img[r] = make_int4(1, 0, 0, 0);   // one live slot: step 1 expands slot 0 only (every slot is [bos] with zero state there)
    }
}

// One step for image n = blockIdx.x (include/lrcn_nbest.h gives the rules):
//   candidates c = i * K + j of the live slots i < nlive, value cum[i] + topv[i][j]; ranked by value, descending, ties to the lower c;
//   the walk takes them in rank order: eos -> the pool, any other word -> the next free live slot, until K slots are full (eos
//   candidates number at most one per slot, so the walk never passes rank 2K);
//   the last step (current = nword + 1) flushes the live slots into the pool, truncated; then the early-stop test.
// Thread 0 walks and keeps the pool (<= 2K inserts of <= K entries in LDS); the other work is spread over the workgroup.
__global__ __launch_bounds__(256) void nbest_update_kernel(const int32_t *topi, const float *topv, NbestState s) {
    __shared__ float cv[kMaxK * kMaxK];
    __shared__ int ct[kMaxK * kMaxK];               // the candidates' words
    __shared__ int sel[2 * kMaxK];
    __shared__ float ps[kMaxK], pl[kMaxK];          // pool: score, logp
    __shared__ int pst[kMaxK], pln[kMaxK];          // pool: storage row, length (tokens incl. bos)
    __shared__ int psrc[kMaxK], ptok[kMaxK];        // pool entries new in this step: source slot and last token (psrc -1: older entry)
    __shared__ int fsrc[kMaxK], ftok[kMaxK];        // the new live slots: parent slot, word
    __shared__ float fcum[kMaxK];
    __shared__ int sh_nf, sh_cnt, sh_done;
    const int n = blockIdx.x, tid = threadIdx.x, K = s.K, L = s.L, cur = s.current;
    const int r0 = n * K;
    const int4 im = s.img[n];
    if (im.z) {   // done, frozen: identity parent, eos fed (its results are already written)
        for (int k = tid; k < K; k += blockDim.x) {
            s.parent[r0 + k] = r0 + k;
            s.last[r0 + k] = s.eos;
        }
        return;
    }
    const int nl = im.x, C = nl * K, W = C < 2 * K ? C : 2 * K;
    for (int c = tid; c < C; c += blockDim.x) {   // topi / topv rows r0 .. r0 + nl - 1 are contiguous: candidate c is entry r0 * K + c
        cv[c] = s.cum[r0 + c / K] + topv[(int64_t)r0 * K + c];
        ct[c] = topi[(int64_t)r0 * K + c];
    }
    const int cnt0 = im.y;
    for (int k = tid; k < cnt0; k += blockDim.x) {
        const int4 e = s.pool[r0 + k];
        ps[k] = __int_as_float(e.x);
        pl[k] = __int_as_float(e.y);
        pst[k] = e.z;
        pln[k] = e.w;
        psrc[k] = -1;
    }
    __syncthreads();
    for (int c = tid; c < C; c += blockDim.x) {
        const float v = cv[c];
        int rank = 0;
        for (int q = 0; q < C; ++q) rank += (cv[q] > v) || (cv[q] == v && q < c);
        if (rank < W) sel[rank] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int cnt = cnt0, nf = 0;
        unsigned long long used = 0;   // storage rows referenced by the pool (2K <= 64)
        for (int k = 0; k < cnt; ++k) used |= 1ull << pst[k];
        for (int q = 0; q < W; ++q) {
            const int c = sel[q], i = c / K, tok = ct[c];
            if (tok == s.eos) {
                pool_insert(cv[c], i, tok, s.lp_cur, K, cur + 1, cnt, used, ps, pl, pst, pln, psrc, ptok);
            } else {
                fsrc[nf] = i; ftok[nf] = tok; fcum[nf] = cv[c];
                if (++nf == K) break;
            }
        }
        int done = 0;
        if (cur > s.nword) {   // the last step: the live hypotheses enter the pool truncated, in slot order
            for (int f = 0; f < nf; ++f) pool_insert(fcum[f], fsrc[f], ftok[f], s.lp_cur, K, cur + 1, cnt, used, ps, pl, pst, pln, psrc, ptok);
            done = 1;
        } else if (nf == 0) {
            done = 1;
        } else if (cnt == K) {   // exact: no live hypothesis can still reach a score above the pool's worst (cum never grows, L <= nword + 1)
            float best = fcum[0];
            for (int f = 1; f < nf; ++f) best = fmaxf(best, fcum[f]);
            done = ps[K - 1] >= best / s.lp_max;
        }
        sh_nf = nf;
        sh_cnt = cnt;
        sh_done = done;
    }
    __syncthreads();
    const int nf = sh_nf, cnt = sh_cnt, done = sh_done;
    for (int k = tid; k < K; k += blockDim.x) {
        const bool live = !done && k < nf;
        s.parent[r0 + k] = live ? r0 + fsrc[k] : r0 + k;
        s.last[r0 + k] = live ? ftok[k] : s.eos;
        s.cum[r0 + k] = live ? fcum[k] : -INFINITY;
    }
    for (int k = tid; k < cnt; k += blockDim.x) s.pool[r0 + k] = make_int4(__float_as_int(ps[k]), __float_as_int(pl[k]), pst[k], pln[k]);
    if (tid == 0) s.img[n] = make_int4(done ? 0 : nf, cnt, done, 0);
    const int P = cur + 1;   // positions 0 .. cur of a history written this step
    if (!done) {
        // new histories: the parent slot's tokens, then the word; new pool entries: the source slot's tokens, then eos / the word
        for (int e = tid; e < nf * P; e += blockDim.x) {
            const int k = e / P, pos = e - k * P;
            s.seq_out[(int64_t)(r0 + k) * L + pos] = pos < cur ? s.seq_in[(int64_t)(r0 + fsrc[k]) * L + pos] : ftok[k];
        }
        for (int e = tid; e < cnt * P; e += blockDim.x) {
            const int k = e / P, pos = e - k * P;
            if (psrc[k] >= 0)
                s.store[((int64_t)n * 2 * K + pst[k]) * L + pos] = pos < cur ? s.seq_in[(int64_t)(r0 + psrc[k]) * L + pos] : ptok[k];
        }
        return;
    }
    // done: the pool becomes the image's results (rows past the pool: length 0, zeros, -inf), read from where each entry's tokens are
    for (int e = tid; e < K * L; e += blockDim.x) {
        const int k = e / L, pos = e - k * L;
        int32_t t = 0;
        if (k < cnt && pos < pln[k]) {
            if (psrc[k] < 0) t = s.store[((int64_t)n * 2 * K + pst[k]) * L + pos];
            else t = pos < cur ? s.seq_in[(int64_t)(r0 + psrc[k]) * L + pos] : ptok[k];
        }
        s.res_tok[(int64_t)(r0 + k) * L + pos] = t;
    }
    for (int k = tid; k < K; k += blockDim.x) {
        s.res_len[r0 + k] = k < cnt ? pln[k] : 0;
        s.res_logp[r0 + k] = k < cnt ? pl[k] : -INFINITY;
        s.res_score[r0 + k] = k < cnt ? ps[k] : -INFINITY;
    }
    if (tid == 0) atomicAdd(s.ndone, 1);
}

}  // namespace

void k_nbest_init(hipStream_t st, const NbestState &s, int N, int bos) {
    const int R = N * s.K;
    hipLaunchKernelGGL(nbest_init_kernel, dim3((R + 255) / 256), dim3(256), 0, st, s, N, bos);
}
void k_nbest_update(hipStream_t st, const int32_t *topi, const float *topv, const NbestState &s, int N) {
    hipLaunchKernelGGL(nbest_update_kernel, dim3(N), dim3(256), 0, st, topi, topv, s);
}
