// train_kernels.hip -- the kernels only the training step (train.hip, update.hip) launches: token rows, the embedding gradient (scatter, sparse
// export, ordered sums), dropout mask + reduce of dX2, the shadow-weight pass with and without Adam, multi-tensor Adam, and the gradient-norm
// clipping of include/lrcn_clip.h (sum of squares, control block, the clipped forms of both Adam kernels), and the next-input kernel of
// scheduled sampling (include/lrcn_sched.h).
#include "kernel_util.h"
#include "draw.h"

namespace {

__global__ void build_tokens_kernel(const int32_t *tokens, int T, int B, int V, int32_t *tok_in, int32_t *tok_tgt, double *zero_acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && zero_acc) *zero_acc = 0.0;  // the log-likelihood accumulator of softmax_xent (saves a memset launch)
    const int S = T + 1;
    if (i >= S * B) return;
    const int s = i / B, b = i - s * B;
    int in = (s == 0) ? 1 : tokens[(s - 1) * B + b];
    int tg = (s < T) ? tokens[s * B + b] : 0;
    // out-of-range ids would fault the gather (the reference raises BoundsError, lrcn.jl:556/569): clamp to unk so that nothing
    // faults, and raise the sticky flag zero_acc[1] -- the next synchronising call (lrcn_last_loss / loss_host / lrcn_sync)
    // reports LRCN_EINVAL
    if ((unsigned)in >= (unsigned)V || (unsigned)tg >= (unsigned)V) {
        if (zero_acc) zero_acc[1] = 1.0;
        if ((unsigned)in >= (unsigned)V) in = 2;
        if ((unsigned)tg >= (unsigned)V) tg = 2;
    }
    tok_in[i] = in;
    tok_tgt[i] = tg;
}

// The length-aware sibling (include/lrcn_varlen.h): step s of row b is active for s <= lens[b].  Active steps are built exactly as above
// (with lens[b] in T's place); an inactive step gets the input eos and the target -1, and reads nothing from `tokens`.
__global__ void build_tokens_var_kernel(const int32_t *tokens, const int32_t *lens, int T, int B, int V, int32_t *tok_in, int32_t *tok_tgt,
                                        double *zero_acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && zero_acc) *zero_acc = 0.0;
    const int S = T + 1;
    if (i >= S * B) return;
    const int s = i / B, b = i - s * B;
    const int len = lens[b];
    if (s > len) {
        tok_in[i] = 0;
        tok_tgt[i] = -1;
        return;
    }
    int in = (s == 0) ? 1 : tokens[(s - 1) * B + b];
    int tg = (s < len) ? tokens[s * B + b] : 0;
    if ((unsigned)in >= (unsigned)V || (unsigned)tg >= (unsigned)V) {  // as build_tokens_kernel: clamp to unk, raise the sticky flag
        if (zero_acc) zero_acc[1] = 1.0;
        if ((unsigned)in >= (unsigned)V) in = 2;
        if ((unsigned)tg >= (unsigned)V) tg = 2;
    }
    tok_in[i] = in;
    tok_tgt[i] = tg;
}

// ---- scheduled sampling (include/lrcn_sched.h): the input of row b at step s1 = a.s_next, after the logits of step s1 - 1 ----
// One 256-thread workgroup per row; every branch is uniform over the workgroup (lens[b], the coin and the temperature are per row).
//   s1 > lens[b]   tok_in holds eos (k_build_tokens_var): gather that row.
//   coin           u of Philox counter (0xFFFFFFFF, s1, 0xFFFFFFFF, row0 + b) -- every thread computes the same word; no fire: the gold word
//                  of tok_in, and the logits row is NOT read.
//   fire           the row's maximum (the row staged in LDS up to V = 15360: `stage`, 60 KB of dynamic LDS, two workgroups per CU), then the
//                  Gumbel argmax of draw.h over the columns within 20 * temp of it, noise counter (j >> 2, s1, 0, row0 + b); the winner
//                  goes to tok_in and counts as drawn.  No log-sum-exp: the draw needs none.
// Then the word's embedding row into Xemb row s1*B + b, times the dropout multiplier of step s1 (d: none in LRCN-1f, whose concat applies it).
template <typename T> __global__ __launch_bounds__(256) void sched_next_input_kernel(const SchedNext a, int stage) {
    extern __shared__ float srow[];
    __shared__ float shf[4];
    __shared__ float shv[4];
    __shared__ int shi[4];
    const int b = blockIdx.x, tid = threadIdx.x, s1 = a.s_next;
    const int64_t m = (int64_t)s1 * a.B + b;
    int tok = a.tok_in[m];
    if (s1 <= a.lens[b]) {
        const uint32_t row = a.row0 + (uint32_t)b;
        const uint32_t x = philox4x32_10(0xFFFFFFFFu, (uint32_t)s1, 0xFFFFFFFFu, row, a.k0, a.k1).x[0];
        const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
        const bool fire = u < a.eps;
        if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.cnt), 1ull);
        if (fire) {
            const float *g = a.logits + (int64_t)b * a.ld_l;
            const float *z = stage ? srow : g;
            const float mx = row_max_stage(g, a.V, stage, srow, shf);   // (its barriers also publish srow)
            const float thr = a.temp > 0.0f ? mx - GUMBEL_PRUNE * a.temp : mx;
            float bs, bz;
            int bc;
            gumbel_argmax(z, a.V, a.temp, thr, (uint32_t)s1, 0u, row, a.k0, a.k1, [](float, int) { return true; }, bs, bc, bz);
            block_best(bs, bc, shv, shi);
            tok = (unsigned)bc < (unsigned)a.V ? bc : 2;   // the row's maximum is admitted; only an all-NaN row admits no column: unk
            if (tid == 0) {
                a.tok_in[m] = tok;
                atomicAdd(reinterpret_cast<unsigned long long *>(a.cnt) + 1, 1ull);
            }
        }
    }
    const T *src = reinterpret_cast<const T *>(a.wembT) + (int64_t)tok * a.ld_w;
    T *dst = reinterpret_cast<T *>(a.xemb) + m * a.ld_x;
    for (int e = tid; e < a.E; e += 256) dst[e] = from_f32<T>(to_f32(src[e]) * drop_mult(a.d, s1, b, e, a.B, a.E));
}
__global__ void sched_stats_set_kernel(long long *cnt, long long eligible, long long drawn) {
    cnt[0] = eligible;
    cnt[1] = drawn;
}

// ---- embedding gradient, E-contiguous form (dual of the gather, lrcn.jl:556/569 under AutoGrad) ----
// The Wembed gradient of the ABI is V x E column-major (memory [E][V]): a row of dXemb scattered straight into it touches E different
// cache lines per token (64 lanes -> 64 lines per wave instruction).  Instead: (1) rows are summed per token into a ROW-MAJOR f32
// staging array stage[V][ld] -- lanes run along e, 256-byte coalesced atomics (or ordered sums, below) -- and (2) one dense transpose
// writes every element of the column-major gradient (no memset) and puts the zeros back into the staging rows it found non-zero.
__global__ __launch_bounds__(256) void embed_scatter_rm_kernel(const float *dxemb, int64_t ld_dx, const int32_t *tok_in, int S, int B, int E,
                                                               DropSpec d, float *stage, int64_t ld_s) {
    const int m = blockIdx.x;
    const int s = m / B, b = m - s * B;
    float *dst = stage + (int64_t)tok_in[m] * ld_s;
    const float *src = dxemb + (int64_t)m * ld_dx;
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        const float v = src[e] * drop_mult(d, s, b, e, B, E);
        if (v != 0.0f) atomicAdd(dst + e, v);
    }
}
// Sparse exchange of the embedding gradient (data parallelism): a rank's contribution to d Wembed is its (T+1) B rows of d(x_lstm) (dropout
// multiplier applied) with their token ids -- 1.5 MB at 32 rows against the 42.6 MB dense V x E gradient.  This kernel writes those rows
// E-contiguous into the caller's buffer; the ranks all-gather rows + ids and every rank sums ALL of them in one fixed order
// (rank_token_rows_kernel + embed_segsum_kernel below: bit-identical results on every rank, as an all-reduce would give).
__global__ __launch_bounds__(256) void embed_rows_export_kernel(const float *dxemb, int64_t ld_dx, int S, int B, int E, DropSpec d, float *out) {
    const int m = blockIdx.x;
    const int s = m / B, b = m - s * B;
    const float *src = dxemb + (int64_t)m * ld_dx;
    float *dst = out + (int64_t)m * E;
    for (int e = threadIdx.x; e < E; e += blockDim.x) dst[e] = src[e] * drop_mult(d, s, b, e, B, E);
}
// LRCN_OPT_DETERMINISTIC: the rows grouped by token, each token's rows in row order -- a stable counting sort, integer arithmetic only.  Row m
// goes to position #{rows with a smaller token} + #{earlier rows with its token}; each block ranks 64 rows against all M tokens (in LDS,
// its 4 waves a quarter of them each).  Key = token << 32 | segment length << 16 | row, the length (the token's row count) only at the
// token's first position and 0 elsewhere.  M <= 8192.
__global__ __launch_bounds__(256) void rank_token_rows_kernel(const int32_t *tok_in, int M, unsigned long long *keys_out) {
    extern __shared__ unsigned stok[];
    __shared__ int part[3][4][64];
    for (int i = threadIdx.x; i < M; i += blockDim.x) stok[i] = (unsigned)tok_in[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + lane;
    const unsigned t = m < M ? stok[m] : 0u;
    const int q = (M + 3) / 4, j0 = w * q, j1 = min(M, j0 + q);
    int less = 0, eq_before = 0, eq = 0;
#pragma unroll 8
    for (int j = j0; j < j1; ++j) {
        const unsigned u = stok[j];
        less += u < t;
        eq += u == t;
        eq_before += (u == t) & (j < m);
    }
    part[0][w][lane] = less;
    part[1][w][lane] = eq_before;
    part[2][w][lane] = eq;
    __syncthreads();
    if (w == 0 && m < M) {
        for (int k = 1; k < 4; ++k) {
            less += part[0][k][lane];
            eq_before += part[1][k][lane];
            eq += part[2][k][lane];
        }
        keys_out[less + eq_before] = ((unsigned long long)t << 32) | ((unsigned long long)(eq_before == 0 ? eq : 0) << 16) | (unsigned)m;
    }
}
// ... and one workgroup per (token, 256-column slice) adds the token's rows: their row ids go to LDS 512 at a time, wave w takes rows w, w + 8,
// ... of the segment in order, and the eight partial sums are added in wave order -- a fixed summation order, plain stores.  (A segment can
// hold a tenth of all rows: Zipf tokens.)
__global__ __launch_bounds__(512) void embed_segsum_kernel(const float *dxemb, int64_t ld_dx, const unsigned long long *keys, int M, int B, int E,
                                                          DropSpec d, float *stage, int64_t ld_s) {
    __shared__ float part[8][256];
    __shared__ int rows[512];
    const int i = blockIdx.x;
    const unsigned long long head = keys[i];
    const int n = (int)((head >> 16) & 0xFFFF);
    if (n == 0) return;  // not the first row of its token (uniform over the block)
    const unsigned tok = (unsigned)(head >> 32);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e0 = blockIdx.y * 256 + lane * 4;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < n; c0 += 512) {  // n is uniform over the block: so are the barriers
        const int cn = min(512, n - c0);
        __syncthreads();  // the previous chunk's ids have been read
        if ((int)threadIdx.x < cn) rows[threadIdx.x] = (int)(keys[i + c0 + threadIdx.x] & 0xFFFF);
        __syncthreads();
        if (e0 < E) {
#pragma unroll 4
            for (int j = w; j < cn; j += 8) {
                const int m = rows[j];
                const int s = m / B, b = m - s * B;
                const float *src = dxemb + (int64_t)m * ld_dx;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e0 + k < E) acc[k] += src[e0 + k] * drop_mult(d, s, b, e0 + k, B, E);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[w][lane * 4 + k] = acc[k];
    __syncthreads();
    if (w == 0 && e0 < E) {
        float *dst = stage + (int64_t)tok * ld_s;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = part[0][lane * 4 + k];
#pragma unroll
            for (int r = 1; r < 8; ++r) t += part[r][lane * 4 + k];
            if (e0 + k < E) dst[e0 + k] = t;
        }
    }
}
// stage[V][ld_s] (row-major, f32) -> dwembed (V x E column-major: [E][V]); every element of dwembed is written; non-zero staging
// values are replaced by zeros, so the staging array is all-zero again when the kernel ends.  64 x 64 tiles through LDS.
__global__ __launch_bounds__(256) void embed_stage_to_grad_kernel(float *stage, int64_t ld_s, int V, int E, float *dwembed) {
    __shared__ float tile[64][65];
    const int tv = (V + 63) / 64;
    const int v0 = (blockIdx.x % tv) * 64, e0 = (blockIdx.x / tv) * 64;
    const int q = threadIdx.x & 15, rr = threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int v = v0 + rr + 16 * i, e = e0 + 4 * q;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (v < V) {
            float *src = stage + (int64_t)v * ld_s + e;
            if (e + 3 < E && (ld_s % 4) == 0) {
                const float4 f = *reinterpret_cast<const float4 *>(src);
                x[0] = f.x; x[1] = f.y; x[2] = f.z; x[3] = f.w;
                if (f.x != 0.f || f.y != 0.f || f.z != 0.f || f.w != 0.f) *reinterpret_cast<float4 *>(src) = make_float4(0.f, 0.f, 0.f, 0.f);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e + k < E) {
                        x[k] = src[k];
                        if (x[k] != 0.f) src[k] = 0.f;
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[rr + 16 * i][4 * q + k] = x[k];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = e0 + rr + 16 * i, v = v0 + 4 * q;
        if (e >= E) continue;
        float *dst = dwembed + (int64_t)e * V + v;
        if (v + 3 < V && (V % 4) == 0) {
            *reinterpret_cast<float4 *>(dst) = make_float4(tile[4 * q][rr + 16 * i], tile[4 * q + 1][rr + 16 * i], tile[4 * q + 2][rr + 16 * i],
                                                           tile[4 * q + 3][rr + 16 * i]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v + k < V) dst[k] = tile[4 * q + k][rr + 16 * i];
        }
    }
}

template <typename T>
__global__ void dx2_mask_reduce_kernel(T *dx2, int64_t ld, int S, int B, int nl, int nr, DropSpec d, float *dxcnn, int64_t ld_dxc) {
    const int b = blockIdx.x, j = blockIdx.y * blockDim.x + threadIdx.x;
    if (j >= nl + nr) return;
    float acc = 0.0f;
    for (int s = 0; s < S; ++s) {
        T *p = dx2 + (int64_t)(s * B + b) * ld + j;
        const float v = to_f32(*p) * drop_mult(d, s, b, j, B, nl + nr);
        *p = from_f32<T>(v);
        acc += v;
    }
    if (j >= nl) dxcnn[(int64_t)b * ld_dxc + (j - nl)] = acc;
}

// All shadow weights of one model in ONE launch (was 8 cast_rows + 9 transpose launches per step): for every 32 x 32 tile of
// a parameter's memory image [R][C] (f32) write the direct copy split at column `cs` (dA[r][c], dB[r][c - cs]) and / or the
// transposed copy (tA[c][r], tB[c - cs][r]) in T.  Padding columns of the destinations are never touched (zero since allocation).
template <typename T, bool ADAM = false, bool CLIP = false> __global__ __launch_bounds__(256) void prepare_weights_kernel(const PrepPlan plan) {
    // 64 x 64 tiles, 16 bytes in / 8 bytes out per thread access (bf16); generic element-wise path for f32 shadows and edges
    __shared__ float tile[64][65];
    // CLIP: a skipped step (non-finite norm) leaves w, m and v alone and STILL writes the shadows below, from the unchanged parameters
    float clip_scale = 1.0f;
    bool clip_skip = false;
    if constexpr (CLIP) {
        clip_scale = plan.clip->scale;
        clip_skip = plan.clip->skip != 0;
    }
    // plan.total tiles walked by gridDim.x workgroups (the launchers start one workgroup per tile)
    for (int bid = blockIdx.x; bid < plan.total; bid += gridDim.x) {
    if (bid != (int)blockIdx.x) __syncthreads();  // the previous tile's transposed stores have read `tile`
    int d = 0;
#pragma unroll
    for (int k = 1; k < PREP_MAX; ++k)
        if (k < plan.n && bid >= plan.d[k].tile0) d = k;
    const PrepDesc &P = plan.d[d];
    const int t = bid - P.tile0;
    const int tc = (P.C + 63) / 64;
    const int r0 = (t / tc) * 64, c0 = (t % tc) * 64;
    const int q = threadIdx.x & 15, rr = threadIdx.x >> 4;  // 16 column quads x 16 row groups
    const bool vec = (P.C % 4) == 0 && (P.cs % 4) == 0;
    auto al = [](const void *p, int64_t ld) { return (reinterpret_cast<uintptr_t>(p) % (4 * sizeof(T))) == 0 && (ld % 4) == 0; };
    const bool alA = al(P.dA, P.ldA), alB = al(P.dB, P.ldB), altA = al(P.tA, P.ldtA), altB = al(P.tB, P.ldtB);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + rr + 16 * i, c = c0 + 4 * q;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (r < P.R) {
            if (vec && c + 3 < P.C) {
                const float4 x = *reinterpret_cast<const float4 *>(P.src + (int64_t)r * P.C + c);
                v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < P.C) v[k] = P.src[(int64_t)r * P.C + c + k];
            }
            if (ADAM && !(CLIP && clip_skip)) {  // update! on the loaded values (the arithmetic of adam_kernel), written back before the shadows are made
                const int64_t o = (int64_t)r * P.C + c;
                float gg[4] = {0.f, 0.f, 0.f, 0.f}, mm[4] = {0.f, 0.f, 0.f, 0.f}, vv[4] = {0.f, 0.f, 0.f, 0.f};
                const bool v4 = vec && c + 3 < P.C;
                if (v4) {
                    const float4 a = *reinterpret_cast<const float4 *>(P.g + o), b = *reinterpret_cast<const float4 *>(P.m + o),
                                 d4 = *reinterpret_cast<const float4 *>(P.v + o);
                    gg[0] = a.x; gg[1] = a.y; gg[2] = a.z; gg[3] = a.w;
                    mm[0] = b.x; mm[1] = b.y; mm[2] = b.z; mm[3] = b.w;
                    vv[0] = d4.x; vv[1] = d4.y; vv[2] = d4.z; vv[3] = d4.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < P.C) { gg[k] = P.g[o + k]; mm[k] = P.m[o + k]; vv[k] = P.v[o + k]; }
                }
                if constexpr (CLIP) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) gg[k] = __fmul_rn(gg[k], clip_scale);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    mm[k] = plan.b1 * mm[k] + (1.0f - plan.b1) * gg[k];
                    vv[k] = plan.b2 * vv[k] + (1.0f - plan.b2) * gg[k] * gg[k];
                    v[k] -= plan.lr * (mm[k] / plan.c1) / (sqrtf(vv[k] / plan.c2) + plan.eps);
                }
                float *w = const_cast<float *>(P.src);
                if (v4) {
                    *reinterpret_cast<float4 *>(P.m + o) = make_float4(mm[0], mm[1], mm[2], mm[3]);
                    *reinterpret_cast<float4 *>(P.v + o) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    *reinterpret_cast<float4 *>(w + o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < P.C) { P.m[o + k] = mm[k]; P.v[o + k] = vv[k]; w[o + k] = v[k]; }
                }
            }
            if (P.dG) {  // gate-interleaved rows of the B side (element-wise: the destination is written once per step, 8 MB)
                const int rg = (r % P.giH) * 4 + r / P.giH;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k >= P.cs && c + k < P.C) reinterpret_cast<T *>(P.dG)[(int64_t)rg * P.ldG + (c + k - P.cs)] = from_f32<T>(v[k]);
            }
            const bool sideA = c + 3 < P.cs, sideB = c >= P.cs;
            const int rd = P.permH > 0 ? (r % P.permH) * 4 + r / P.permH : r;  // destination row of the direct copies
            if (vec && c + 3 < P.C && sideA && alA) {
                if (P.dA) store4(reinterpret_cast<T *>(P.dA) + (int64_t)rd * P.ldA + c, v);
            } else if (vec && c + 3 < P.C && sideB && alB) {
                if (P.dB) store4(reinterpret_cast<T *>(P.dB) + (int64_t)rd * P.ldB + (c - P.cs), v);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cc = c + k;
                    if (cc >= P.C) continue;
                    if (cc < P.cs) {
                        if (P.dA) reinterpret_cast<T *>(P.dA)[(int64_t)rd * P.ldA + cc] = from_f32<T>(v[k]);
                    } else if (P.dB) {
                        reinterpret_cast<T *>(P.dB)[(int64_t)rd * P.ldB + (cc - P.cs)] = from_f32<T>(v[k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[rr + 16 * i][4 * q + k] = v[k];
    }
    if (!P.tA && !P.tB) continue;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + rr + 16 * i;  // source column = destination row
        if (c >= P.C) continue;
        T *dst = nullptr;
        if (c < P.cs) {
            if (P.tA) dst = reinterpret_cast<T *>(P.tA) + (int64_t)c * P.ldtA;
        } else if (P.tB) {
            dst = reinterpret_cast<T *>(P.tB) + (int64_t)(c - P.cs) * P.ldtB;
        }
        if (!dst) continue;
        const int r = r0 + 4 * q;
        if (r + 3 < P.R && (c < P.cs ? altA : altB)) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = tile[4 * q + k][rr + 16 * i];
            store4(dst + r, v);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (r + k < P.R) dst[r + k] = from_f32<T>(tile[4 * q + k][rr + 16 * i]);
        }
    }
    }
}

template <bool CLIP>
__global__ void adam_kernel(AdamTensors t, float lr, float b1, float b2, float eps, float c1, float c2, const ClipCtl *clip) {
    float scale = 1.0f;
    if constexpr (CLIP) {
        if (clip->skip) return;  // a non-finite norm: w, m and v stay as they are
        scale = clip->scale;
    }
    const int k = blockIdx.y;
    const int64_t n = t.n[k];
    float *w = t.w[k], *m = t.m[k], *v = t.v[k];
    const float *g = t.g[k];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = CLIP ? __fmul_rn(g[i], scale) : g[i];
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        w[i] -= lr * (mi / c1) / (sqrtf(vi / c2) + eps);
    }
}

__global__ void mul_f32_kernel(const float *a, const float *b, int64_t n, float *out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = a[i] * b[i];
}

// Stage 1 of k_sumsq: workgroup blockIdx.x of run blockIdx.y owns the 4-element groups [x cg, (x + 1) cg) of the run, cg = ceil(groups /
// kSumsqParts).  A float's square is exact in double, so only the additions round.
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const SumsqArgs a, double *parts) {
    __shared__ double red[256];
    const int e = blockIdx.y, tid = threadIdx.x;
    const float *__restrict__ g = a.g[e];
    const int64_t n = a.n[e];
    const int64_t groups = (n + 3) / 4, full = n / 4;
    const int64_t cg = (groups + kSumsqParts - 1) / kSumsqParts;
    const int64_t q0 = (int64_t)blockIdx.x * cg;
    const int64_t q1 = q0 + cg < groups ? q0 + cg : groups, qf = q1 < full ? q1 : full;
    const bool al = (reinterpret_cast<uintptr_t>(g) % 16) == 0;
    double acc = 0.0;
    if (al) {
#pragma unroll 8
        for (int64_t q = q0 + tid; q < qf; q += 256) {
            const float4 x = *reinterpret_cast<const float4 *>(g + 4 * q);
            const double d0 = x.x, d1 = x.y, d2 = x.z, d3 = x.w;
            acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
        }
    } else {  // the same groups, the same order, element loads
#pragma unroll 4
        for (int64_t q = q0 + tid; q < qf; q += 256) {
            const double d0 = g[4 * q], d1 = g[4 * q + 1], d2 = g[4 * q + 2], d3 = g[4 * q + 3];
            acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
        }
    }
    if (full < groups && full >= q0 && full < q1 && (full - q0) % 256 == tid) {  // the run's last, partial group: its owner's last one
        for (int64_t i = 4 * full; i < n; ++i) {
            const double d = g[i];
            acc += d * d;
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) parts[(int64_t)a.slot[e] * kSumsqParts + blockIdx.x] = red[0];
}
// Stage 2: one workgroup per run, one lane adds the run's partials in index order.
__global__ __launch_bounds__(256) void sumsq_final_kernel(const SumsqArgs a, const double *parts, ClipCtl *ctl) {
    __shared__ double red[kSumsqParts];
    const int slot = a.slot[blockIdx.x];
    for (int i = threadIdx.x; i < kSumsqParts; i += 256) red[i] = parts[(int64_t)slot * kSumsqParts + i];
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < kSumsqParts; ++i) s += red[i];
        ctl->slot[slot] = s;
    }
}
__global__ void clip_set_kernel(ClipCtl *ctl, int n_slots, float max_norm) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < n_slots; ++k) s += ctl->slot[k];
    const double norm = sqrt(s);
    const int skip = isfinite(norm) ? 0 : 1;
    const bool clip = !skip && norm > (double)max_norm;
    ctl->norm = norm;
    ctl->skip = skip;
    ctl->scale = clip ? (float)((double)max_norm / norm) : 1.0f;
    ctl->steps += 1;
    ctl->clipped += clip ? 1 : 0;
    ctl->skipped += skip;
}

}  // namespace
// ---------------------------------------------------------------- launchers
void k_build_tokens(hipStream_t st, const int32_t *tokens, int T, int B, int V, int32_t *tok_in, int32_t *tok_tgt, double *zero_acc) {
    const int n = (T + 1) * B;
    hipLaunchKernelGGL(build_tokens_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, tokens, T, B, V, tok_in, tok_tgt, zero_acc);
}
void k_build_tokens_var(hipStream_t st, const int32_t *tokens, const int32_t *lens, int T, int B, int V, int32_t *tok_in, int32_t *tok_tgt,
                        double *zero_acc) {
    const int n = (T + 1) * B;
    hipLaunchKernelGGL(build_tokens_var_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, tokens, lens, T, B, V, tok_in, tok_tgt, zero_acc);
}
void k_sched_next_input(hipStream_t st, int dtype, const SchedNext &a) {
    const int stage = a.V <= 15360;   // as k_sample_rows: 60 KB of LDS (+ the static few bytes: under the default 64 KB limit)
    DISPATCH_T(dtype, hipLaunchKernelGGL(sched_next_input_kernel<T>, dim3(a.B), dim3(256), stage ? sizeof(float) * a.V : 0, st, a, stage));
}
void k_sched_stats_set(hipStream_t st, long long *cnt, long long eligible, long long drawn) {
    hipLaunchKernelGGL(sched_stats_set_kernel, dim3(1), dim3(1), 0, st, cnt, eligible, drawn);
}
void k_embed_rows_export(hipStream_t st, const float *dxemb, int64_t ld_dx, int S, int B, int E, DropSpec d, float *out) {
    hipLaunchKernelGGL(embed_rows_export_kernel, dim3(S * B), dim3(256), 0, st, dxemb, ld_dx, S, B, E, d, out);
}
bool k_embed_scatter_rm(hipStream_t st, const float *dxemb, int64_t ld_dx, const int32_t *tok_in, int S, int B, int E, int V, DropSpec d,
                        float *stage, int64_t ld_s, float *dwembed, unsigned long long *sort_keys) {
    const int M = S * B;
    if (sort_keys) {  // ordered sums
        if (M > 8192) return false;
        hipLaunchKernelGGL(rank_token_rows_kernel, dim3(cdiv(M, 64)), dim3(256), sizeof(unsigned) * (size_t)M, st, tok_in, M, sort_keys);
        hipLaunchKernelGGL(embed_segsum_kernel, dim3(M, cdiv(E, 256)), dim3(512), 0, st, dxemb, ld_dx, sort_keys, M, B, E, d, stage, ld_s);
    } else {
        hipLaunchKernelGGL(embed_scatter_rm_kernel, dim3(M), dim3(256), 0, st, dxemb, ld_dx, tok_in, S, B, E, d, stage, ld_s);
    }
    hipLaunchKernelGGL(embed_stage_to_grad_kernel, dim3(cdiv(V, 64) * cdiv(E, 64)), dim3(256), 0, st, stage, ld_s, V, E, dwembed);
    return true;
}
void k_dx2_mask_reduce(hipStream_t st, int dtype, void *dx2, int64_t ld, int S, int B, int nl, int nr, DropSpec d, float *dxcnn,
                       int64_t ld_dxc) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(dx2_mask_reduce_kernel<T>, dim3(B, cdiv(nl + nr, 256)), dim3(256), 0, st, (T *)dx2, ld, S, B, nl,
                                         nr, d, dxcnn, ld_dxc));
}
void k_prepare_weights(hipStream_t st, int dtype, PrepPlan &plan) {
    const int tiles = number_tiles(plan, 0);
    if (tiles == 0) return;
    plan.total = tiles;
    DISPATCH_T(dtype, hipLaunchKernelGGL(prepare_weights_kernel<T>, dim3(tiles), dim3(256), 0, st, plan));
}
void k_adam_shadows(hipStream_t st, int dtype, PrepPlan &plan, int step, float lr, float b1, float b2, float eps) {
    const int tiles = number_tiles(plan, 0);
    if (tiles == 0) return;
    plan.lr = lr; plan.b1 = b1; plan.b2 = b2; plan.eps = eps;
    plan.c1 = (float)(1.0 - pow((double)b1, (double)step));
    plan.c2 = (float)(1.0 - pow((double)b2, (double)step));
    plan.total = tiles;
    if (plan.clip) {
        DISPATCH_T(dtype, hipLaunchKernelGGL((prepare_weights_kernel<T, true, true>), dim3(tiles), dim3(256), 0, st, plan));
    } else {
        DISPATCH_T(dtype, hipLaunchKernelGGL((prepare_weights_kernel<T, true>), dim3(tiles), dim3(256), 0, st, plan));
    }
}
void k_adam(hipStream_t st, const AdamTensors &t, int step, float lr, float b1, float b2, float eps, const ClipCtl *clip) {
    const float c1 = (float)(1.0 - pow((double)b1, (double)step)), c2 = (float)(1.0 - pow((double)b2, (double)step));
    if (clip)
        hipLaunchKernelGGL(adam_kernel<true>, dim3(1024, 9), dim3(256), 0, st, t, lr, b1, b2, eps, c1, c2, clip);
    else
        hipLaunchKernelGGL(adam_kernel<false>, dim3(1024, 9), dim3(256), 0, st, t, lr, b1, b2, eps, c1, c2, clip);
}
void k_sumsq(hipStream_t st, const SumsqArgs &a, double *parts, ClipCtl *ctl) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(kSumsqParts, a.count), dim3(256), 0, st, a, parts);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(a.count), dim3(256), 0, st, a, parts, ctl);
}
void k_clip_set(hipStream_t st, ClipCtl *ctl, int n_slots, float max_norm) {
    hipLaunchKernelGGL(clip_set_kernel, dim3(1), dim3(64), 0, st, ctl, n_slots, max_norm);
}
void k_mul_f32(hipStream_t st, const float *a, const float *b, int64_t n, float *out) {
    hipLaunchKernelGGL(mul_f32_kernel, dim3(grid1d(n)), dim3(256), 0, st, a, b, n, out);
}
