// diverse.hip -- the per-step bookkeeping of diverse beam search (lrcn_beam_diverse_batch, include/lrcn_diverse.h): the n-best beam's
// slots, pools and early stop (nbest.hip) per group of K' = K / G, the groups of an image walked in order so that a group's proposals are
// penalised by the words the groups before it took at this step.  One workgroup per image; the step's log-probability top-K at the full
// width K comes in topi / topv, which by the header's lemma holds every row's K' penalised best.
#include "kernels.h"

#include "common.h"
#include "nbest_pool.h"

namespace {

constexpr int kMaxK = 32;

__global__ void diverse_init_kernel(DiverseState d, int N, int bos) {
    const NbestState &s = d.nb;
    const int R = N * s.K;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
        const_cast<int32_t *>(s.seq_in)[(int64_t)r * s.L] = bos;
        s.last[r] = bos;
        s.parent[r] = r;
        s.cum[r] = 0.0f;
        if (r < N * d.G) s.img[r] = make_int4(1, 0, 0, 0);   // one live slot per group: step 1 expands the group's slot 0 only
        if (r < N) d.done[r] = 0;
    }
}

// One step for image n = blockIdx.x.  For each group g in order (a uniform trip count; every barrier is reached by the whole workgroup,
// and what differs between groups is loop bounds, which are block-uniform):
//   A1  entry (i, j) of the live rows i < nl: a = fmaf(-lambda, cnt(word), logp), cnt from the image's penalised-word list in LDS
//   A2  each entry's rank in its row by (a descending, word ascending); rank < K' makes candidate i * K' + rank with the selection value
//       cum_i + a and the true value cum_i + logp
//   B   the candidates' ranks by (selection value descending, index ascending), by counting
//   C   thread 0 walks them as the n-best kernel does -- eos to the group's pool, any other word to the next free slot, both with the
//       true value -- flushes at the last step, tests satisfaction, and adds the new slots' words to the penalised list
// then the whole workgroup writes the slots, pools and histories of all groups, and the results once the image is done.
__global__ __launch_bounds__(256) void diverse_update_kernel(const int32_t *topi, const float *topv, DiverseState d) {
    __shared__ float av[kMaxK * kMaxK], alp[kMaxK * kMaxK];   // a row's penalised values and log-probabilities
    __shared__ int aw[kMaxK * kMaxK];
    __shared__ float csel[kMaxK * kMaxK], cv[kMaxK * kMaxK];  // candidates: selection value, true value
    __shared__ int ct[kMaxK * kMaxK];
    __shared__ int sel[2 * kMaxK];
    __shared__ float scum[kMaxK];
    __shared__ float ps[kMaxK], pl[kMaxK];          // the G pools, group g at g * K': score, logp
    __shared__ int pst[kMaxK], pln[kMaxK];          // storage row (of the group's 2K'), length
    __shared__ int psrc[kMaxK], ptok[kMaxK];        // entries new in this step: source slot (group-local) and last token (psrc -1: older)
    __shared__ int fsrc[kMaxK], ftok[kMaxK];        // the new live slots, group g at g * K': parent slot (group-local), word
    __shared__ float fcum[kMaxK];
    __shared__ int pw[kMaxK], pc[kMaxK];            // penalised words of this step and their counts
    __shared__ int g_nl[kMaxK], g_nf[kMaxK], g_cnt[kMaxK], g_sat[kMaxK];
    __shared__ int sh_npw;
    const NbestState &s = d.nb;
    const int n = blockIdx.x, tid = threadIdx.x, K = s.K, L = s.L, cur = s.current, G = d.G, Kp = K / G;
    const int r0 = n * K;
    if (d.done[n]) {   // done, frozen: identity parent, eos fed (its results are already written)
        for (int k = tid; k < K; k += blockDim.x) {
            s.parent[r0 + k] = r0 + k;
            s.last[r0 + k] = s.eos;
        }
        return;
    }
    for (int k = tid; k < K; k += blockDim.x) {
        const int g = k / Kp, kl = k - g * Kp;
        const int4 im = s.img[n * G + g];
        if (kl == 0) {
            g_nl[g] = im.x;
            g_cnt[g] = im.y;
        }
        scum[k] = s.cum[r0 + k];
        if (kl < im.y) {
            const int4 e = s.pool[r0 + k];
            ps[k] = __int_as_float(e.x);
            pl[k] = __int_as_float(e.y);
            pst[k] = e.z;
            pln[k] = e.w;
        }
        psrc[k] = -1;
    }
    if (tid == 0) sh_npw = 0;
    __syncthreads();
    for (int g = 0; g < G; ++g) {
        const int nl = g_nl[g], rg = r0 + g * Kp, A = nl * K, C = nl * Kp, W = C < 2 * Kp ? C : 2 * Kp;
        const int npw = sh_npw;
        for (int e = tid; e < A; e += blockDim.x) {   // the group's rows rg .. rg + nl - 1 are contiguous in topi / topv
            const int w = topi[(int64_t)rg * K + e];
            const float lp = topv[(int64_t)rg * K + e];
            int cnt = 0;
            for (int q = 0; q < npw; ++q) cnt = pw[q] == w ? pc[q] : cnt;
            av[e] = fmaf(-d.lambda, (float)cnt, lp);
            alp[e] = lp;
            aw[e] = w;
        }
        for (int c = tid; c < C; c += blockDim.x) {   // (a candidate or rank that no entry claims -- NaN logits only -- stays in bounds)
            csel[c] = -INFINITY; cv[c] = -INFINITY; ct[c] = s.eos;
        }
        for (int q = tid; q < W; q += blockDim.x) sel[q] = 0;
        __syncthreads();
        for (int e = tid; e < A; e += blockDim.x) {
            const int i = e / K, b = i * K, w = aw[e];
            const float a = av[e];
            int rank = 0;
            for (int q = 0; q < K; ++q) rank += (av[b + q] > a) || (av[b + q] == a && aw[b + q] < w);
            if (rank < Kp) {
                const int c = i * Kp + rank;
                csel[c] = scum[g * Kp + i] + a;
                cv[c] = scum[g * Kp + i] + alp[e];
                ct[c] = w;
            }
        }
        __syncthreads();
        for (int c = tid; c < C; c += blockDim.x) {
            const float v = csel[c];
            int rank = 0;
            for (int q = 0; q < C; ++q) rank += (csel[q] > v) || (csel[q] == v && q < c);
            if (rank < W) sel[rank] = c;
        }
        __syncthreads();
        if (tid == 0) {
            const int o = g * Kp;
            int cnt = g_cnt[g], nf = 0;
            unsigned long long used = 0;   // the group's storage rows referenced by its pool (2K' <= 64)
            for (int k = 0; k < cnt; ++k) used |= 1ull << pst[o + k];
            for (int q = 0; q < W; ++q) {
                const int c = sel[q], i = c / Kp, tok = ct[c];
                if (tok == s.eos) {
                    pool_insert(cv[c], i, tok, s.lp_cur, Kp, cur + 1, cnt, used, ps + o, pl + o, pst + o, pln + o, psrc + o, ptok + o);
                } else {
                    fsrc[o + nf] = i; ftok[o + nf] = tok; fcum[o + nf] = cv[c];
                    if (++nf == Kp) break;
                }
            }
            int m = sh_npw;   // the words just taken penalise the groups after this one (a dead group has nf = 0)
            for (int f = 0; f < nf; ++f) {
                int q = 0;
                while (q < m && pw[q] != ftok[o + f]) ++q;
                if (q == m) {
                    pw[m] = ftok[o + f]; pc[m] = 0;
                    ++m;
                }
                ++pc[q];
            }
            sh_npw = m;
            int sat = 0;
            if (cur > s.nword) {   // the last step: the live hypotheses enter the pool truncated, in slot order
                for (int f = 0; f < nf; ++f)
                    pool_insert(fcum[o + f], fsrc[o + f], ftok[o + f], s.lp_cur, Kp, cur + 1, cnt, used, ps + o, pl + o, pst + o, pln + o, psrc + o, ptok + o);
            } else if (nf > 0 && cnt == Kp) {   // exact, as in the n-best kernel: the pool can no longer change
                float best = fcum[o];
                for (int f = 1; f < nf; ++f) best = fmaxf(best, fcum[o + f]);
                sat = ps[o + Kp - 1] >= best / s.lp_max;
            }
            g_nf[g] = nf;
            g_cnt[g] = cnt;
            g_sat[g] = sat;
        }
        __syncthreads();
    }
    int done = 1;   // every group dead or satisfied, or the last step (all threads read the same LDS: uniform)
    if (cur <= s.nword)
        for (int g = 0; g < G; ++g) done &= g_nf[g] == 0 || g_sat[g];
    for (int k = tid; k < K; k += blockDim.x) {
        const int g = k / Kp, kl = k - g * Kp;
        const bool live = !done && kl < g_nf[g];
        s.parent[r0 + k] = live ? r0 + g * Kp + fsrc[k] : r0 + k;
        s.last[r0 + k] = live ? ftok[k] : s.eos;
        s.cum[r0 + k] = live ? fcum[k] : -INFINITY;
        if (kl < g_cnt[g]) s.pool[r0 + k] = make_int4(__float_as_int(ps[k]), __float_as_int(pl[k]), pst[k], pln[k]);
        if (kl == 0) s.img[n * G + g] = make_int4(done ? 0 : g_nf[g], g_cnt[g], g_nf[g] == 0, g_sat[g]);
    }
    const int P = cur + 1;   // positions 0 .. cur of a history written this step
    if (!done) {
        // new histories: the parent slot's tokens, then the word; new pool entries: the source slot's tokens, then eos
        for (int e = tid; e < K * P; e += blockDim.x) {
            const int k = e / P, pos = e - k * P, g = k / Kp, kl = k - g * Kp;
            if (kl < g_nf[g]) s.seq_out[(int64_t)(r0 + k) * L + pos] = pos < cur ? s.seq_in[(int64_t)(r0 + g * Kp + fsrc[k]) * L + pos] : ftok[k];
            if (kl < g_cnt[g] && psrc[k] >= 0)
                s.store[((int64_t)n * 2 * K + g * 2 * Kp + pst[k]) * L + pos] = pos < cur ? s.seq_in[(int64_t)(r0 + g * Kp + psrc[k]) * L + pos] : ptok[k];
        }
        return;
    }
    // done: the pools become the image's results, group-major (rows past a group's pool: length 0, zeros, -inf)
    for (int e = tid; e < K * L; e += blockDim.x) {
        const int k = e / L, pos = e - k * L, g = k / Kp, kl = k - g * Kp;
        int32_t t = 0;
        if (kl < g_cnt[g] && pos < pln[k]) {
            if (psrc[k] < 0) t = s.store[((int64_t)n * 2 * K + g * 2 * Kp + pst[k]) * L + pos];
            else t = pos < cur ? s.seq_in[(int64_t)(r0 + g * Kp + psrc[k]) * L + pos] : ptok[k];
        }
        s.res_tok[(int64_t)(r0 + k) * L + pos] = t;
    }
    for (int k = tid; k < K; k += blockDim.x) {
        const int g = k / Kp, kl = k - g * Kp;
        const bool has = kl < g_cnt[g];
        s.res_len[r0 + k] = has ? pln[k] : 0;
        s.res_logp[r0 + k] = has ? pl[k] : -INFINITY;
        s.res_score[r0 + k] = has ? ps[k] : -INFINITY;
    }
    if (tid == 0) {
        d.done[n] = 1;
        atomicAdd(s.ndone, 1);
    }
}

}  // namespace

void k_diverse_init(hipStream_t st, const DiverseState &s, int N, int bos) {
    const int R = N * s.nb.K;
    hipLaunchKernelGGL(diverse_init_kernel, dim3((R + 255) / 256), dim3(256), 0, st, s, N, bos);
}
void k_diverse_update(hipStream_t st, const int32_t *topi, const float *topv, const DiverseState &s, int N) {
    hipLaunchKernelGGL(diverse_update_kernel, dim3(N), dim3(256), 0, st, topi, topv, s);
}
