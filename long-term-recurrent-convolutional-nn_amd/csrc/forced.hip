// forced.hip -- the per-step bookkeeping of forced-word beam search (lrcn_beam_forced_batch, include/lrcn_forced.h): the n-best beam's
// slots, pool and early stop (nbest.hip) with S = 2^C banks of K slots per image, one bank per state of the forced-word automaton, and ONE
// pool per image.  One workgroup per image, modelled on diverse.hip with banks in place of groups; the step's stay proposals come in
// topi / topv [N*S*K][K] and its move values in s.move [N*S*K][C*A] (forced_topk_rows_kernel, constrain.hip).
#include "kernels.h"

#include "common.h"
#include "nbest_pool.h"

namespace {

constexpr int kMaxRows = 32;                 // S * K, the rows of an image
constexpr int kMaxBanks = 1 << kForcedMaxSets;
constexpr int kMaxCand = kMaxRows * kMaxRows;   // of one bank: K*K stay + popcount(b) * K * A moves <= 1024 under S * K <= 32

__global__ void forced_init_kernel(ForcedState d, int N, int bos) {
    const NbestState &s = d.nb;
    const int S = 1 << d.C, R = N * S * s.K;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < R; r += gridDim.x * blockDim.x) {
        const_cast<int32_t *>(s.seq_in)[(int64_t)r * s.L] = bos;
        s.last[r] = bos;
        s.parent[r] = r;
        s.cum[r] = 0.0f;
        if (r < N * S) s.img[r] = make_int4((r & (S - 1)) == 0 ? 1 : 0, 0, 0, 0);   // step 1 expands row 0 of bank 0 only; empty pool
        if (r < N) d.done[r] = 0;
    }
}

// One step for image n = blockIdx.x.  The banks are walked in a block-uniform loop (a bank outside the image's present sets is skipped by
// every thread alike); per bank b:
//   A  the candidates that target b: entry (i, j) of its live rows' stay proposals, value cum_i + logp, index i*(K + C*A) + j; and for
//      every set c in b the moves of the live rows of bank b ^ 1<<c, value cum_i + move, index i*(K + C*A) + K + c*A + a (a move that is
//      not proposed -- no word, or -inf -- keeps its place with the word -1 and the value -inf, behind every real candidate)
//   B  their ranks by (value descending, index ascending), by counting; the indices are distinct, so the ranks are a permutation
//   C  thread 0 walks them as the n-best kernel does: eos to the image's pool (only the accepting bank proposes it), any other word to
//      the bank's next free slot.  At most K eos candidates (one per row) precede the K-th slot: the walk never passes rank 2K.
// All candidates are made from the state before the step: the banks do not interact.  Then thread 0 flushes the accepting bank at the last
// step and tests the stop, and the whole workgroup writes parents (which may point into another bank), tokens, cum, histories, the pool's
// storage and -- once the image is done -- the results, in the first K rows of the image.
__global__ __launch_bounds__(256) void forced_update_kernel(const int32_t *topi, const float *topv, ForcedState d) {
    __shared__ float cv[kMaxCand];
    __shared__ int ct[kMaxCand], cx[kMaxCand];      // the candidates' words and indices
    __shared__ int sel[2 * kMaxRows];
    __shared__ float scum[kMaxRows];
    __shared__ float ps[kMaxRows], pl[kMaxRows];    // pool: score, logp
    __shared__ int pst[kMaxRows], pln[kMaxRows];    // pool: storage row (of the image's 2K), length
    __shared__ int psrc[kMaxRows], ptok[kMaxRows];  // entries new in this step: source row (image-local) and last token (psrc -1: older)
    __shared__ int fsrc[kMaxRows], ftok[kMaxRows];  // the new live slots, bank b at b * K: parent row (image-local), word
    __shared__ float fcum[kMaxRows];
    __shared__ int b_nl[kMaxBanks], b_nf[kMaxBanks];
    __shared__ int fw[kForcedMaxWords];
    __shared__ int sh_cnt, sh_done;
    const NbestState &s = d.nb;
    const int n = blockIdx.x, tid = threadIdx.x, K = s.K, L = s.L, cur = s.current, C = d.C, A = d.A, CA = C * A, S = 1 << C, SK = S * K;
    const int stride = K + CA, r0 = n * SK;
    if (d.done[n]) {   // done, frozen: identity parent, eos fed (its results are already written)
        for (int k = tid; k < SK; k += blockDim.x) {
            s.parent[r0 + k] = r0 + k;
            s.last[r0 + k] = s.eos;
        }
        return;
    }
    const int cnt0 = s.img[n * S].y;
    for (int k = tid; k < SK; k += blockDim.x) {
        scum[k] = s.cum[r0 + k];
        psrc[k] = -1;
        if (k < cnt0) {
            const int4 e = s.pool[r0 + k];
            ps[k] = __int_as_float(e.x);
            pl[k] = __int_as_float(e.y);
            pst[k] = e.z;
            pln[k] = e.w;
        }
    }
    if (tid < S) b_nl[tid] = s.img[n * S + tid].x;
    if (tid < CA) fw[tid] = d.words[(int64_t)n * CA + tid];
    __syncthreads();
    int full = 0;   // the image's present sets (every thread reads the same LDS: uniform)
    for (int q = 0; q < CA; ++q) full |= fw[q] >= 0 ? 1 << (q / A) : 0;
    int cnt = cnt0;                 // thread 0's: the pool count and the storage rows its entries reference (2K <= 64)
    unsigned long long used = 0;
    if (tid == 0)
        for (int k = 0; k < cnt; ++k) used |= 1ull << pst[k];
    for (int b = 0; b < S; ++b) {
        if (b & ~full) {   // dead for this image
            if (tid == 0) b_nf[b] = 0;
            continue;
        }
        const int nstay = b_nl[b] * K;
        for (int e = tid; e < nstay; e += blockDim.x) {   // the bank's live rows are contiguous in topi / topv
            const int i = b * K + e / K, j = e - (e / K) * K;
            cv[e] = scum[i] + topv[(int64_t)(r0 + b * K) * K + e];
            ct[e] = topi[(int64_t)(r0 + b * K) * K + e];
            cx[e] = i * stride + j;
        }
        int Cn = nstay;
        for (int c = 0; c < C; ++c) {
            if (!((b >> c) & 1)) continue;
            const int src = b ^ (1 << c), m = b_nl[src] * A;
            for (int e = tid; e < m; e += blockDim.x) {
                const int sl = e / A, al = e - sl * A, i = src * K + sl, w = fw[c * A + al];
                const float mv = d.move[(int64_t)(r0 + i) * CA + c * A + al];
                const bool ok = w >= 0 && mv > -INFINITY;
                cv[Cn + e] = ok ? scum[i] + mv : -INFINITY;
                ct[Cn + e] = ok ? w : -1;
                cx[Cn + e] = i * stride + K + c * A + al;
            }
            Cn += m;
        }
        const int W = Cn < 2 * K ? Cn : 2 * K;
        __syncthreads();
        for (int c = tid; c < Cn; c += blockDim.x) {
            const float v = cv[c];
            const int x = cx[c];
            int rank = 0;
            for (int q = 0; q < Cn; ++q) rank += (cv[q] > v) || (cv[q] == v && cx[q] < x);
            if (rank < W) sel[rank] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int nf = 0;
            for (int q = 0; q < W; ++q) {
                const int c = sel[q], tok = ct[c], i = cx[c] / stride;
                if (tok < 0) continue;   // not proposed
                if (tok == s.eos) {
                    pool_insert(cv[c], i, tok, s.lp_cur, K, cur + 1, cnt, used, ps, pl, pst, pln, psrc, ptok);
                } else {
                    fsrc[b * K + nf] = i; ftok[b * K + nf] = tok; fcum[b * K + nf] = cv[c];
                    if (++nf == K) break;
                }
            }
            b_nf[b] = nf;
        }
        __syncthreads();   // the next bank reuses the candidate arrays
    }
    if (tid == 0) {
        int done = 0, any = 0;
        for (int b = 0; b < S; ++b) any += b_nf[b];
        if (cur > s.nword) {   // the last step: the accepting bank's live hypotheses enter the pool truncated, in slot order
            for (int f = 0; f < b_nf[full]; ++f)
                pool_insert(fcum[full * K + f], fsrc[full * K + f], ftok[full * K + f], s.lp_cur, K, cur + 1, cnt, used, ps, pl, pst, pln, psrc, ptok);
            done = 1;
        } else if (any == 0) {
            done = 1;
        } else if (cnt == K) {   // exact: no live hypothesis of any bank can still reach a score above the pool's worst
            float best = -INFINITY;
            for (int b = 0; b < S; ++b)
                for (int f = 0; f < b_nf[b]; ++f) best = fmaxf(best, fcum[b * K + f]);
            done = ps[K - 1] >= best / s.lp_max;
        }
        sh_cnt = cnt;
        sh_done = done;
    }
    __syncthreads();
    const int pc = sh_cnt, done = sh_done;
    for (int k = tid; k < SK; k += blockDim.x) {
        const int b = k / K, kl = k - b * K;
        const bool live = !done && kl < b_nf[b];
        s.parent[r0 + k] = live ? r0 + fsrc[k] : r0 + k;
        s.last[r0 + k] = live ? ftok[k] : s.eos;
        s.cum[r0 + k] = live ? fcum[k] : -INFINITY;
        if (kl == 0) s.img[n * S + b] = make_int4(done ? 0 : b_nf[b], b == 0 ? pc : 0, 0, 0);
    }
    for (int k = tid; k < pc; k += blockDim.x) s.pool[r0 + k] = make_int4(__float_as_int(ps[k]), __float_as_int(pl[k]), pst[k], pln[k]);
    const int P = cur + 1;   // positions 0 .. cur of a history written this step
    if (!done) {
        // new histories: the parent row's tokens, then the word; new pool entries: the source row's tokens, then eos
        for (int e = tid; e < SK * P; e += blockDim.x) {
            const int k = e / P, pos = e - k * P, b = k / K, kl = k - b * K;
            if (kl < b_nf[b]) s.seq_out[(int64_t)(r0 + k) * L + pos] = pos < cur ? s.seq_in[(int64_t)(r0 + fsrc[k]) * L + pos] : ftok[k];
        }
        for (int e = tid; e < pc * P; e += blockDim.x) {
            const int k = e / P, pos = e - k * P;
            if (psrc[k] >= 0)
                s.store[((int64_t)n * 2 * K + pst[k]) * L + pos] = pos < cur ? s.seq_in[(int64_t)(r0 + psrc[k]) * L + pos] : ptok[k];
        }
        return;
    }
    // done: the pool becomes the image's results, in its first K rows (rows past the pool: length 0, zeros, -inf)
    for (int e = tid; e < K * L; e += blockDim.x) {
        const int k = e / L, pos = e - k * L;
        int32_t t = 0;
        if (k < pc && pos < pln[k]) {
            if (psrc[k] < 0) t = s.store[((int64_t)n * 2 * K + pst[k]) * L + pos];
            else t = pos < cur ? s.seq_in[(int64_t)(r0 + psrc[k]) * L + pos] : ptok[k];
        }
        s.res_tok[(int64_t)(r0 + k) * L + pos] = t;
    }
    for (int k = tid; k < K; k += blockDim.x) {
        s.res_len[r0 + k] = k < pc ? pln[k] : 0;
        s.res_logp[r0 + k] = k < pc ? pl[k] : -INFINITY;
        s.res_score[r0 + k] = k < pc ? ps[k] : -INFINITY;
    }
    if (tid == 0) {
        d.done[n] = 1;
        atomicAdd(s.ndone, 1);
    }
}

}  // namespace

void k_forced_init(hipStream_t st, const ForcedState &s, int N, int bos) {
    const int R = N * (1 << s.C) * s.nb.K;
    hipLaunchKernelGGL(forced_init_kernel, dim3((R + 255) / 256), dim3(256), 0, st, s, N, bos);
}
void k_forced_update(hipStream_t st, const int32_t *topi, const float *topv, const ForcedState &s, int N) {
    hipLaunchKernelGGL(forced_update_kernel, dim3(N), dim3(256), 0, st, topi, topv, s);
}
