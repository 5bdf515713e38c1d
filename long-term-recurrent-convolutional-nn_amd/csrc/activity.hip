// activity.hip -- LRCN activity recognition (include/lrcn_activity.h): one LSTM layer over per-frame features and a per-step softmax
// head whose distributions are averaged over each clip's real frames.  The recurrence is the caption model's (host.h lstm_recurrence_fwd /
// _bwd: the fused bf16 step kernels of lstm_fused.hip or GEMM + k_lstm_fwd / k_lstm_bwd), with launch_gemm, k_colsum and k_transpose_multi
// around it; the new kernels are
//   act_frames_kernel -- the caller's clip-major column-major f32 features -> time-major rows X [t*B + b][f] (T) and, for the weight
//                        gradient, their transpose X' [f][t*B + b] (T, zero K padding), in one pass through an LDS tile
//   act_head_kernel   -- one workgroup per clip, its T logit rows in step order: log-softmax, the masked NLL term, dlogits, per-step
//                        probabilities and the clip average (no atomics: the loss and the probabilities are reproducible bit for bit)
//   act_loss_sum_kernel -- the per-clip NLL terms summed in clip order (double)
// and, for dropout on the two non-recurrent connections (include/lrcn_act_dropout.h; the multipliers are drop_mult's of kernel_util.h),
//   act_frames_kernel<T, true> -- the same tile pass with the input multiplier applied as the tile is loaded (X and X' from one masked tile)
//   act_head_drop_kernel -- Hall -> the head's masked operand Hd [m][j] and, for dWout, its transpose Hd' (zero K padding), one LDS tile pass
//   act_dh_mask_kernel   -- dHall *= m_out (f32), between the dh GEMM and the reverse recurrence
#include <algorithm>
#include <cmath>

#include "../../include/lrcn_act_dropout.h"
#include "host.h"
#include "kernel_util.h"

using namespace lrcn_impl;

namespace {

// X[m][f] = feats[f * N + b * Tn + t] with m = t * B + b, N = Tn * B; XT (optional) [f][m] with zeros for M <= m < ldxt.
// Grid: (F / 64 tiles, m tiles of 64 up to M (X only) or ldxt (with XT)).
// DROP: v *= drop_mult(d, t, b, f) as the tile is loaded, for m < M only (the zero fill of XT stays zero, no mask is evaluated there).
template <typename T, bool DROP>
__global__ __launch_bounds__(256) void act_frames_kernel(const float *feats, int F, int Tn, int B, T *X, int64_t ldx, T *XT, int64_t ldxt,
                                                         DropSpec d) {
    __shared__ float tile[64][65];
    const int f0 = blockIdx.x * 64, m0 = blockIdx.y * 64, tid = threadIdx.x;
    const int M = Tn * B;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + 256 * k, fr = idx >> 6, mr = idx & 63;
        const int f = f0 + fr, m = m0 + mr;
        float v = 0.0f;
        if (f < F && m < M) {
            const int t = m / B, b = m - t * B;
            v = feats[(int64_t)f * M + (int64_t)b * Tn + t];
            if (DROP) v *= drop_mult(d, t, b, f, B, F);
        }
        tile[fr][mr] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + 256 * k, mr = idx >> 6, fr = idx & 63;
        const int f = f0 + fr, m = m0 + mr;
        if (f < F && m < M) X[(int64_t)m * ldx + f] = from_f32<T>(tile[fr][mr]);
    }
    if (!XT) return;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + 256 * k, fr = idx >> 6, mr = idx & 63;
        const int f = f0 + fr, m = m0 + mr;
        if (f < F && m < ldxt) XT[(int64_t)f * ldxt + m] = from_f32<T>(tile[fr][mr]);
    }
}

// Hd[m][j] = Hall[m][j] * m_out(t, b, j) with m = t * B + b (T, one rounding after the f32 product); HdT (optional) [j][m] with zeros for
// M <= m < ldt.  Hall is only read.  Grid: (H / 64 tiles, m tiles of 64 up to M (Hd only) or ldt (with HdT)).
template <typename T>
__global__ __launch_bounds__(256) void act_head_drop_kernel(const T *Hall, int64_t ldh, int H, int Tn, int B, DropSpec d, T *Hd, T *HdT,
                                                            int64_t ldt) {
    __shared__ float tile[64][65];
    const int j0 = blockIdx.x * 64, m0 = blockIdx.y * 64, tid = threadIdx.x;
    const int M = Tn * B;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + 256 * k, mr = idx >> 6, jr = idx & 63;
        const int j = j0 + jr, m = m0 + mr;
        float v = 0.0f;
        if (j < H && m < M) {
            const int t = m / B, b = m - t * B;
            const T r = from_f32<T>(to_f32(Hall[(int64_t)m * ldh + j]) * drop_mult(d, t, b, j, B, H));
            Hd[(int64_t)m * ldh + j] = r;
            v = to_f32(r);
        }
        tile[mr][jr] = v;
    }
    __syncthreads();
    if (!HdT) return;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = tid + 256 * k, jr = idx >> 6, mr = idx & 63;
        const int j = j0 + jr, m = m0 + mr;
        if (j < H && m < ldt) HdT[(int64_t)j * ldt + m] = from_f32<T>(tile[mr][jr]);
    }
}

// dH[m][j] *= m_out(t, b, j), f32 [M][H] dense
__global__ __launch_bounds__(256) void act_dh_mask_kernel(float *dH, int H, int Tn, int B, DropSpec d) {
    const int64_t n = (int64_t)Tn * B * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int m = (int)(i / H), j = (int)(i - (int64_t)m * H);
        const int t = m / B, b = m - t * B;
        dH[i] *= drop_mult(d, t, b, j, B, H);
    }
}

// block-wide max / sum of 256 threads; every thread gets the same value (combined from the four waves' lane-0 results in a fixed order)
__device__ __forceinline__ float act_block_max(float v, float *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    __syncthreads();
    return r;
}
__device__ __forceinline__ float act_block_sum(float v, float *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// One workgroup per clip b over rows m = t * B + b, t = 0 .. Tn-1 in order.  NQ = columns per thread (C <= 256 * NQ).
//   t < len: p = softmax(z); frame_probs[(b*Tn + t)*C + c] = p; clip += p; dlog[m][c] = (p - [c == label]) * scale; nll += lse - z[label]
//   t >= len: frame_probs and dlog rows are zero.  dlog columns [C, ldd) are written as zeros (K padding of the dh GEMM).
// loss_clip[b] = nll (double, summed in step order); clip_probs[b*C + c] = clip / len.
template <typename T, int NQ>
__global__ __launch_bounds__(256) void act_head_kernel(const float *logits, int64_t ldl, int Tn, int B, int C, const int32_t *labels,
                                                       const int32_t *lens, float scale, T *dlog, int64_t ldd, double *loss_clip,
                                                       float *clip_probs, float *frame_probs) {
    __shared__ float sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = lens[b];
    const int lab = labels ? labels[b] : -1;
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0f;
    double nll = 0.0;
    for (int t = 0; t < Tn; ++t) {
        const int64_t m = (int64_t)t * B + b;
        float *fp = frame_probs ? frame_probs + ((int64_t)b * Tn + t) * C : nullptr;
        T *dl = dlog ? dlog + m * ldd : nullptr;
        if (t >= len) {
            if (fp)
                for (int c = tid; c < C; c += 256) fp[c] = 0.0f;
            if (dl)
                for (int c = tid; c < ldd; c += 256) dl[c] = from_f32<T>(0.0f);
            continue;
        }
        const float *row = logits + m * ldl;
        float z[NQ];
        float mx = -INFINITY;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = tid + 256 * q;
            z[q] = c < C ? row[c] : -INFINITY;
            mx = fmaxf(mx, z[q]);
        }
        mx = act_block_max(mx, sh);
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = tid + 256 * q;
            z[q] = c < C ? expf(z[q] - mx) : 0.0f;
            s += z[q];
        }
        s = act_block_sum(s, sh);
        const float inv = 1.0f / s;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = tid + 256 * q;
            if (c < C) {
                const float p = z[q] * inv;
                acc[q] += p;
                if (fp) fp[c] = p;
                if (dl) dl[c] = from_f32<T>((p - (c == lab ? 1.0f : 0.0f)) * scale);
            }
        }
        if (dl)
            for (int c = C + tid; c < ldd; c += 256) dl[c] = from_f32<T>(0.0f);
        if (tid == 0 && lab >= 0) nll += (double)(mx + logf(s)) - (double)row[lab];
    }
    if (clip_probs) {
        const float il = 1.0f / (float)len;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c = tid + 256 * q;
            if (c < C) clip_probs[(int64_t)b * C + c] = acc[q] * il;
        }
    }
    if (tid == 0 && loss_clip) loss_clip[b] = nll;
}

__global__ void act_loss_sum_kernel(const double *loss_clip, int B, double *out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += loss_clip[b];
        out[0] = s;
    }
}
}  // namespace

struct lrcn_act {
    lrcn_act_config cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    int dt = GEMM_T_F32;
    size_t esz = 4;
    int64_t ldF = 0, ldH = 0, ld4H = 0, ldC = 0, ldMmax = 0;
    std::vector<void *> allocs;
    void *zero_page = nullptr, *ws = nullptr;
    size_t ws_bytes = 0;
    // shadows of the parameters (T): W[0:F] rows [4H][ldF], W[F:F+H] [4H][ldH] and its transpose [H][ld4H], Wout [C][ldH] and its transpose [H][ldC]
    void *Wx = nullptr, *Wh = nullptr, *WhT = nullptr, *Wo = nullptr, *WoT = nullptr;
    void *X = nullptr;       // [Mmax][ldF] time-major frames
    void *TA = nullptr;      // [max(4H, C)][ldMmax]: dlog' then dZ'
    void *TB = nullptr;      // [F + 2H][ldMmax]: rows [0, F) X', [F, F+H) h_prev', [F+H, F+2H) h'
    float *Gx = nullptr;     // [Mmax][4H]
    void *acts = nullptr;    // [Mmax][ld4H]
    float *Call = nullptr;   // [Mmax][H]
    void *Hall = nullptr;    // [Mmax][ldH]
    void *Hd = nullptr;      // [Mmax][ldH]: Hall with the output dropout's multipliers, the head's operand (allocated by the first call that drops)
    float *Logits = nullptr; // [Mmax][ldC]
    void *dLog = nullptr;    // [Mmax][ldC]
    float *dHall = nullptr;  // [Mmax][H]
    void *dZ = nullptr;      // [Mmax][ld4H]
    float *dc = nullptr, *dhrec = nullptr;  // [maxB][H]
    double *loss_clip = nullptr, *loss_sum = nullptr;
    int32_t *dmeta = nullptr;  // [2 * maxB]: labels | lens
    int32_t *hmeta = nullptr;  // pinned staging of dmeta
    double *hloss = nullptr;   // pinned
    hipEvent_t up_done = nullptr;
    bool up_pending = false;
};

namespace {

std::string g_act_create_err;

// C[M][N] (+)= A[M][K] B[N][K]' (K: gemm_k), deterministic split-K on the handle's own workspace
int act_gemm(lrcn_act *a, const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc, int M, int N, int K, const float *bias,
             bool beta = false, bool c_is_zero = false) {
    GemmArgs g{};
    g.dtype = a->dt;
    g.A = A; g.lda = lda;
    g.B = B; g.ldb = ldb;
    g.C = C; g.ldc = ldc;
    g.M = M; g.N = N;
    g.K = gemm_k(a->dt, lda, ldb, K);
    g.bias = bias;
    g.c_f32 = 1;
    g.beta = beta;
    g.c_is_zero = c_is_zero;
    g.a_mode = GEMM_A_PLAIN;
    g.out_mode = GEMM_OUT_PLAIN;
    g.zero_page = a->zero_page;
    g.deterministic = a->cfg.deterministic ? 1 : 0;
    g.ws = a->ws;
    g.ws_bytes = a->ws_bytes;
    hipError_t e = launch_gemm(a->stream, g);
    if (e != hipSuccess) FAIL(a, LRCN_EHIP, "gemm M=%d N=%d K=%d: %s", M, N, K, hipGetErrorString(e));
    return LRCN_OK;
}
#define AGEMM(...)                       \
    do {                                 \
        int _r = act_gemm(__VA_ARGS__);  \
        if (_r) return _r;               \
    } while (0)

// the recurrence's plain-form GEMM (host.h lstm_recurrence_*)
auto rec_gemm(lrcn_act *a) {
    return [a](const void *A, int64_t lda, const void *B, int64_t ldb, float *C, int64_t ldc, int M, int N, int K, bool beta, bool c_is_zero) {
        return act_gemm(a, A, lda, B, ldb, C, ldc, M, N, K, nullptr, beta, c_is_zero);
    };
}

template <typename T> void launch_head(hipStream_t st, int nq, const float *logits, int64_t ldl, int Tn, int B, int C, const int32_t *labels,
                                       const int32_t *lens, float scale, void *dlog, int64_t ldd, double *loss_clip, float *clip, float *frame) {
#define ACT_HEAD(Q)                                                                                                                  \
    hipLaunchKernelGGL((act_head_kernel<T, Q>), dim3(B), dim3(256), 0, st, logits, ldl, Tn, B, C, labels, lens, scale, (T *)dlog, ldd, \
                       loss_clip, clip, frame)
    if (nq <= 1) ACT_HEAD(1);
    else if (nq <= 2) ACT_HEAD(2);
    else if (nq <= 4) ACT_HEAD(4);
    else if (nq <= 8) ACT_HEAD(8);
    else ACT_HEAD(16);
#undef ACT_HEAD
}

int check_call(lrcn_act *a, const float *const p[4], const float *feats, const int32_t *labels, const int32_t *lens, int T, int B) {
    if (!p || !p[0] || !p[1] || !p[2] || !p[3]) FAIL(a, LRCN_EINVAL, "null parameter tensor");
    if (!feats) FAIL(a, LRCN_EINVAL, "null feats");
    if (T < 1 || T > a->cfg.max_T) FAIL(a, LRCN_EINVAL, "T=%d outside [1,%d]", T, a->cfg.max_T);
    if (B < 1 || B > a->cfg.max_B) FAIL(a, LRCN_EINVAL, "B=%d outside [1,%d]", B, a->cfg.max_B);
    for (int b = 0; b < B; ++b) {
        if (labels && (labels[b] < 0 || labels[b] >= a->cfg.C)) FAIL(a, LRCN_EINVAL, "labels[%d]=%d outside [0,%d)", b, labels[b], a->cfg.C);
        if (lens && (lens[b] < 1 || lens[b] > T)) FAIL(a, LRCN_EINVAL, "lens[%d]=%d outside [1,%d]", b, lens[b], T);
    }
    return LRCN_OK;
}

// labels (may be NULL) and lens (NULL = T) -> the device's meta array, through the pinned staging buffer (reused once the last upload ran)
int upload_meta(lrcn_act *a, const int32_t *labels, const int32_t *lens, int T, int B) {
    if (a->up_pending) HIPCHK(a, hipEventSynchronize(a->up_done));
    for (int b = 0; b < B; ++b) {
        a->hmeta[b] = labels ? labels[b] : -1;
        a->hmeta[a->cfg.max_B + b] = lens ? lens[b] : T;
    }
    HIPCHK(a, hipMemcpyAsync(a->dmeta, a->hmeta, sizeof(int32_t) * 2 * (size_t)a->cfg.max_B, hipMemcpyHostToDevice, a->stream));
    HIPCHK(a, hipEventRecord(a->up_done, a->stream));
    a->up_pending = true;
    return LRCN_OK;
}

inline bool drops(const DropSpec *d) { return d && (d->mask || d->p > 0.0f); }

// frames -> Gx -> recurrence -> logits.  bwd: also the transposed frames into TB (the weight gradient's operand).
// din / dout (may be NULL or the identity): the multipliers of the frames and of the head's operand (then Hd, and with bwd its transpose in TB).
int act_forward(lrcn_act *a, const float *const p[4], const float *feats, int T, int B, bool bwd, const DropSpec *din = nullptr,
                const DropSpec *dout = nullptr) {
    const int F = a->cfg.F, H = a->cfg.H, C = a->cfg.C, dt = a->dt, M = T * B;
    const int64_t ldF = a->ldF, ldH = a->ldH, ld4H = a->ld4H, ldC = a->ldC, ldM = ld64(M);
    hipStream_t st = a->stream;
    // parameter shadows (W memory [4H][F+H], Wout memory [C][H])
    k_cast_rows(st, dt, p[0], F + H, 4 * H, F, a->Wx, ldF);
    k_cast_rows(st, dt, p[0] + F, F + H, 4 * H, H, a->Wh, ldH);
    k_cast_rows(st, dt, p[2], H, C, H, a->Wo, ldH);
    if (bwd || lstm_fused_on(dt, B, H, ldH, ld4H)) k_transpose(st, dt, 1, p[0] + F, F + H, 4 * H, H, a->WhT, ld4H, 0);
    if (bwd) k_transpose(st, dt, 1, p[2], H, C, H, a->WoT, ldC, 0);
    // frames, time-major (and transposed for dW)
    {
        const dim3 grid(cdiv(F, 64), cdiv(bwd ? ldM : M, 64));
        const DropSpec none{};
#define ACT_FRAMES(TY, DROP, D)                                                                                                  \
    hipLaunchKernelGGL((act_frames_kernel<TY, DROP>), grid, dim3(256), 0, st, feats, F, T, B, (TY *)a->X, ldF,                   \
                       bwd ? (TY *)a->TB : nullptr, ldM, D)
        if (drops(din)) {
            if (dt == GEMM_T_BF16) ACT_FRAMES(bf16_t, true, *din);
            else ACT_FRAMES(float, true, *din);
        } else {
            if (dt == GEMM_T_BF16) ACT_FRAMES(bf16_t, false, none);
            else ACT_FRAMES(float, false, none);
        }
#undef ACT_FRAMES
    }
    KCHK(a, "shadows / frames");
    // input projection of every frame at once: Gx = X W[0:F] + b
    AGEMM(a, a->X, ldF, a->Wx, ldF, a->Gx, 4 * H, M, 4 * H, F, p[1]);
    // recurrence: contracts h only
    if (int r = lstm_recurrence_fwd(a, true, rec_gemm(a), T, B, H, ldH, ld4H, a->Gx, a->Wh, a->acts, a->Call, a->Hall)) return r;
    KCHK(a, "recurrence");
    // logits of every step: z = h Wout + bout, h masked into its second copy Hd under output dropout (Hall stays as the recurrence wrote it)
    const void *Hhead = a->Hall;
    if (drops(dout)) {
        if (!a->Hd) DALLOC(a, a->Hd, a->esz * (size_t)a->cfg.max_B * a->cfg.max_T * ldH);
        const dim3 grid(cdiv(H, 64), cdiv(bwd ? ldM : M, 64));
        void *HdT = bwd ? boff(a->TB, (int64_t)(F + H) * ldM, a->esz) : nullptr;
        if (dt == GEMM_T_BF16)
            hipLaunchKernelGGL(act_head_drop_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t *)a->Hall, ldH, H, T, B, *dout,
                               (bf16_t *)a->Hd, (bf16_t *)HdT, ldM);
        else
            hipLaunchKernelGGL(act_head_drop_kernel<float>, grid, dim3(256), 0, st, (const float *)a->Hall, ldH, H, T, B, *dout,
                               (float *)a->Hd, (float *)HdT, ldM);
        KCHK(a, "head operand");
        Hhead = a->Hd;
    }
    AGEMM(a, Hhead, ldH, a->Wo, ldH, a->Logits, ldC, M, C, H, p[3]);
    return LRCN_OK;
}

// dout (may be NULL or the identity): act_forward has left Hd' in TB rows [F+H, F+2H), and dh takes the same multipliers
int act_backward(lrcn_act *a, const float *const p[4], int T, int B, float *const g[4], const DropSpec *dout = nullptr) {
    (void)p;
    const int F = a->cfg.F, H = a->cfg.H, C = a->cfg.C, dt = a->dt, M = T * B;
    const size_t es = a->esz;
    const int64_t ldH = a->ldH, ld4H = a->ld4H, ldC = a->ldC, ldM = ld64(M);
    const bool det = a->cfg.deterministic != 0;
    hipStream_t st = a->stream;
    auto tr = [&](TrPlan &pl, const void *src, int64_t ld_src, int R, int Cc, void *dst, int shift) {
        TrDesc &d = pl.d[pl.n++];
        d.src = src; d.ld_src = ld_src; d.R = R; d.C = Cc; d.dst = dst; d.ld_dst = ldM; d.shift = shift;
    };
    // head: dWout = h' dlog (Hd' dlog under output dropout), dbout = colsum(dlog), dh = dlog Wout' (.* m_out)
    {
        TrPlan pl{};
        tr(pl, a->dLog, ldC, M, C, a->TA, 0);                                          // dlog' [C][ldM]
        if (!drops(dout)) tr(pl, a->Hall, ldH, M, H, boff(a->TB, (int64_t)(F + H) * ldM, es), 0);  // h' [H][ldM]
        k_transpose_multi(st, dt, pl);
    }
    AGEMM(a, a->TA, ldM, boff(a->TB, (int64_t)(F + H) * ldM, es), ldM, g[2], H, C, H, M, nullptr);
    k_colsum(st, dt, a->dLog, ldC, M, C, g[3], det);
    AGEMM(a, a->dLog, ldC, a->WoT, ldC, a->dHall, H, M, H, C, nullptr);
    if (drops(dout)) hipLaunchKernelGGL(act_dh_mask_kernel, dim3(grid1d((int64_t)M * H)), dim3(256), 0, st, a->dHall, H, T, B, *dout);
    KCHK(a, "head backward");
    // reverse recurrence -> dZ
    if (int r = lstm_recurrence_bwd(a, true, rec_gemm(a), T, B, H, ld4H, a->acts, a->Call, a->dHall, a->WhT, a->dZ)) return r;
    KCHK(a, "recurrence backward");
    // dW = dZ' [X | h_prev] in one GEMM (X' is already in TB rows [0, F)), db = colsum(dZ)
    {
        TrPlan pl{};
        tr(pl, a->dZ, ld4H, M, 4 * H, a->TA, 0);                                                        // dZ' [4H][ldM]
        tr(pl, a->Hall, ldH, M - B, H, boff(a->TB, (int64_t)F * ldM, es), M > B ? B : 0);               // h_prev' (one step later)
        k_transpose_multi(st, dt, pl);
    }
    AGEMM(a, a->TA, ldM, a->TB, ldM, g[0], F + H, 4 * H, F + H, M, nullptr);
    k_colsum(st, dt, a->dZ, ld4H, M, 4 * H, g[1], det);
    KCHK(a, "weight gradients");
    return LRCN_OK;
}

}  // namespace

extern "C" {

int lrcn_act_param_sizes(int F, int H, int C, int64_t sizes[4]) {
    if (F < 1 || H < 1 || C < 1 || !sizes) return LRCN_EINVAL;
    sizes[0] = (int64_t)(F + H) * 4 * H;
    sizes[1] = 4 * (int64_t)H;
    sizes[2] = (int64_t)H * C;
    sizes[3] = C;
    return LRCN_OK;
}

const char *lrcn_act_last_error(const lrcn_act *a) { return a ? a->err.c_str() : g_act_create_err.c_str(); }

void lrcn_act_destroy(lrcn_act *a) {
    if (!a) return;
    DeviceGuard dg(a->cfg.device);
    (void)hipDeviceSynchronize();
    for (void *p : a->allocs) (void)hipFree(p);
    if (a->hmeta) (void)hipHostFree(a->hmeta);
    if (a->hloss) (void)hipHostFree(a->hloss);
    if (a->up_done) (void)hipEventDestroy(a->up_done);
    delete a;
}

static int act_create_impl(lrcn_act *a) {
    const lrcn_act_config &c = a->cfg;
    const int F = c.F, H = c.H, C = c.C;
    a->dt = c.dtype == LRCN_BF16 ? GEMM_T_BF16 : GEMM_T_F32;
    a->esz = a->dt == GEMM_T_BF16 ? 2 : 4;
    a->ldF = ld64(F); a->ldH = ld64(H); a->ld4H = ld64(4 * H); a->ldC = ld64(C);
    const int64_t Mmax = (int64_t)c.max_B * c.max_T;
    a->ldMmax = ld64(Mmax);
    const size_t es = a->esz;
    DALLOC(a, a->zero_page, 4096);
    a->ws_bytes = 48u << 20;
    DALLOC(a, a->ws, a->ws_bytes);
    DALLOC(a, a->Wx, es * 4 * H * a->ldF);
    DALLOC(a, a->Wh, es * 4 * H * a->ldH);
    DALLOC(a, a->WhT, es * H * a->ld4H);
    DALLOC(a, a->Wo, es * C * a->ldH);
    DALLOC(a, a->WoT, es * H * a->ldC);
    DALLOC(a, a->X, es * Mmax * a->ldF);
    DALLOC(a, a->TA, es * (size_t)(4 * H > C ? 4 * H : C) * a->ldMmax);
    DALLOC(a, a->TB, es * (size_t)(F + 2 * H) * a->ldMmax);
    DALLOC(a, a->Gx, sizeof(float) * Mmax * 4 * H);
    DALLOC(a, a->acts, es * Mmax * a->ld4H);
    DALLOC(a, a->Call, sizeof(float) * Mmax * H);
    DALLOC(a, a->Hall, es * Mmax * a->ldH);
    DALLOC(a, a->Logits, sizeof(float) * Mmax * a->ldC);
    DALLOC(a, a->dLog, es * Mmax * a->ldC);
    DALLOC(a, a->dHall, sizeof(float) * Mmax * H);
    DALLOC(a, a->dZ, es * Mmax * a->ld4H);
    DALLOC(a, a->dc, sizeof(float) * c.max_B * H);
    DALLOC(a, a->dhrec, sizeof(float) * c.max_B * H);
    DALLOC(a, a->loss_clip, sizeof(double) * c.max_B);
    DALLOC(a, a->loss_sum, sizeof(double) * 2);
    DALLOC(a, a->dmeta, sizeof(int32_t) * 2 * c.max_B);
    HIPCHK(a, hipHostMalloc((void **)&a->hmeta, sizeof(int32_t) * 2 * c.max_B, hipHostMallocDefault));
    HIPCHK(a, hipHostMalloc((void **)&a->hloss, sizeof(double) * 2, hipHostMallocDefault));
    HIPCHK(a, hipEventCreateWithFlags(&a->up_done, hipEventDisableTiming));
    return LRCN_OK;
}

int lrcn_act_create(const lrcn_act_config *cfg, lrcn_act **out) {
    if (!cfg || !out) {
        g_act_create_err = "null config or output pointer";
        return LRCN_EINVAL;
    }
    *out = nullptr;
    const lrcn_act_config &c = *cfg;
    char buf[256];
    buf[0] = 0;
    if (c.F < 1 || c.H < 1 || c.C < 1) snprintf(buf, sizeof(buf), "F=%d, H=%d, C=%d must be >= 1", c.F, c.H, c.C);
    else if (c.C > 4096) snprintf(buf, sizeof(buf), "C=%d above 4096", c.C);
    else if (c.max_B < 1 || c.max_T < 1) snprintf(buf, sizeof(buf), "max_B=%d, max_T=%d must be >= 1", c.max_B, c.max_T);
    else if (c.dtype != LRCN_F32 && c.dtype != LRCN_BF16) snprintf(buf, sizeof(buf), "dtype=%d must be LRCN_F32 or LRCN_BF16", c.dtype);
    else {
        const int64_t w = std::max(std::max(ld64(c.F), ld64(4 * (int64_t)c.H)), ld64(c.C));
        const int64_t mmax = ld64((int64_t)c.max_B * c.max_T);
        if (mmax * w >= (1ll << 31) || (int64_t)(c.F + 2 * (int64_t)c.H) * mmax >= (1ll << 31) || (int64_t)4 * c.H * ld64(c.F + c.H) >= (1ll << 31))
            snprintf(buf, sizeof(buf), "max_B * max_T = %lld rows of width %lld: above 2^31 elements per buffer", (long long)mmax, (long long)w);
    }
    if (buf[0]) {
        g_act_create_err = buf;
        return LRCN_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || c.device < 0 || c.device >= ndev) {
        g_act_create_err = "device " + std::to_string(c.device) + " not present";
        return LRCN_EINVAL;
    }
    DeviceGuard dg(c.device);
    lrcn_act *a = new lrcn_act();
    a->cfg = c;
    const int r = act_create_impl(a);
    if (r) {
        g_act_create_err = a->err;
        lrcn_act_destroy(a);
        return r;
    }
    *out = a;
    return LRCN_OK;
}

int lrcn_act_set_stream(lrcn_act *a, void *stream) {
    if (!a) return LRCN_EINVAL;
    a->stream = reinterpret_cast<hipStream_t>(stream);
    return LRCN_OK;
}

int lrcn_act_init_weights(lrcn_act *a, float *const p[4], uint64_t seed) {
    if (!a) return LRCN_EINVAL;
    if (!p || !p[0] || !p[1] || !p[2] || !p[3]) FAIL(a, LRCN_EINVAL, "null parameter tensor");
    DeviceGuard dg(a->cfg.device);
    const int F = a->cfg.F, H = a->cfg.H, C = a->cfg.C;
    hipStream_t st = a->stream;
    // the rule of lrcn_init_weights (tensor keys 0 and 7: the caption model's W1 and Wout slots)
    k_init_uniform(st, p[0], (int64_t)(F + H) * 4 * H, (float)std::sqrt(2.0 / ((double)(F + H) + 4.0 * H)), seed, 0);
    k_fill(st, p[1], 4 * (int64_t)H, 0.0f);
    k_fill(st, p[1], H, 1.0f);  // forget-gate bias
    k_init_uniform(st, p[2], (int64_t)H * C, (float)std::sqrt(2.0 / ((double)H + (double)C)), seed, 7);
    k_fill(st, p[3], C, 0.0f);
    KCHK(a, "init_weights");
    return LRCN_OK;
}

// lrcn_act_loss_grad and lrcn_act_loss_grad_drop: din / dout NULL or the identity = the plain call's launches
static int act_loss_grad(lrcn_act *a, const float *const p[4], const float *feats, const int32_t *labels, const int32_t *lens, int T, int B,
                         const DropSpec *din, const DropSpec *dout, float *const g[4], double *loss_host) {
    int r;
    DeviceGuard dg(a->cfg.device);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) total += lens ? lens[b] : T;
    if ((r = upload_meta(a, labels, lens, T, B))) return r;
    const bool bwd = g != nullptr;
    if ((r = act_forward(a, p, feats, T, B, bwd, din, dout))) return r;
    const int nq = cdiv(a->cfg.C, 256);
    const float scale = (float)(1.0 / (double)total);
    if (a->dt == GEMM_T_BF16)
        launch_head<bf16_t>(a->stream, nq, a->Logits, a->ldC, T, B, a->cfg.C, a->dmeta, a->dmeta + a->cfg.max_B, scale, bwd ? a->dLog : nullptr,
                            a->ldC, a->loss_clip, nullptr, nullptr);
    else
        launch_head<float>(a->stream, nq, a->Logits, a->ldC, T, B, a->cfg.C, a->dmeta, a->dmeta + a->cfg.max_B, scale, bwd ? a->dLog : nullptr,
                           a->ldC, a->loss_clip, nullptr, nullptr);
    hipLaunchKernelGGL(act_loss_sum_kernel, dim3(1), dim3(64), 0, a->stream, a->loss_clip, B, a->loss_sum);
    KCHK(a, "head");
    if (bwd && (r = act_backward(a, p, T, B, g, dout))) return r;
    if (loss_host) {
        HIPCHK(a, hipMemcpyAsync(a->hloss, a->loss_sum, sizeof(double), hipMemcpyDeviceToHost, a->stream));
        HIPCHK(a, hipStreamSynchronize(a->stream));
        *loss_host = a->hloss[0] / (double)total;
    }
    return LRCN_OK;
}

static int check_loss_grad(lrcn_act *a, const float *const p[4], const float *feats, const int32_t *labels, const int32_t *lens, int T, int B,
                           float *const g[4]) {
    if (!labels) FAIL(a, LRCN_EINVAL, "null labels");
    if (g && (!g[0] || !g[1] || !g[2] || !g[3])) FAIL(a, LRCN_EINVAL, "null gradient tensor");
    return check_call(a, p, feats, labels, lens, T, B);
}

int lrcn_act_loss_grad(lrcn_act *a, const float *const p[4], const float *feats, const int32_t *labels, const int32_t *lens, int T, int B,
                       float *const g[4], double *loss_host) {
    if (!a) return LRCN_EINVAL;
    if (int r = check_loss_grad(a, p, feats, labels, lens, T, B, g)) return r;
    return act_loss_grad(a, p, feats, labels, lens, T, B, nullptr, nullptr, g, loss_host);
}

int lrcn_act_loss_grad_drop(lrcn_act *a, const float *const p[4], const float *feats, const int32_t *labels, const int32_t *lens, int T, int B,
                            const lrcn_act_dropout *drop, float *const g[4], double *loss_host) {
    if (!a) return LRCN_EINVAL;
    if (int r = check_loss_grad(a, p, feats, labels, lens, T, B, g)) return r;
    if (!drop) return act_loss_grad(a, p, feats, labels, lens, T, B, nullptr, nullptr, g, loss_host);
    if (!(drop->p_in >= 0.0f && drop->p_in < 1.0f)) FAIL(a, LRCN_EINVAL, "p_in=%g outside [0,1)", (double)drop->p_in);
    if (!(drop->p_out >= 0.0f && drop->p_out < 1.0f)) FAIL(a, LRCN_EINVAL, "p_out=%g outside [0,1)", (double)drop->p_out);
    // which = 1 over the F frame columns, which = 2 over the H output columns; a mask given replaces (p, seed) on its side (drop_mult)
    const DropSpec din{drop->p_in, drop->seed, drop->mask_in, 1}, dout{drop->p_out, drop->seed, drop->mask_out, 2};
    return act_loss_grad(a, p, feats, labels, lens, T, B, &din, &dout, g, loss_host);
}

int lrcn_act_predict(lrcn_act *a, const float *const p[4], const float *feats, const int32_t *lens, int T, int B, float *clip_probs,
                     float *frame_probs) {
    if (!a) return LRCN_EINVAL;
    if (!clip_probs) FAIL(a, LRCN_EINVAL, "null clip_probs");
    int r = check_call(a, p, feats, nullptr, lens, T, B);
    if (r) return r;
    DeviceGuard dg(a->cfg.device);
    if ((r = upload_meta(a, nullptr, lens, T, B))) return r;
    if ((r = act_forward(a, p, feats, T, B, false))) return r;
    const int nq = cdiv(a->cfg.C, 256);
    if (a->dt == GEMM_T_BF16)
        launch_head<bf16_t>(a->stream, nq, a->Logits, a->ldC, T, B, a->cfg.C, nullptr, a->dmeta + a->cfg.max_B, 0.0f, nullptr, 0, nullptr,
                            clip_probs, frame_probs);
    else
        launch_head<float>(a->stream, nq, a->Logits, a->ldC, T, B, a->cfg.C, nullptr, a->dmeta + a->cfg.max_B, 0.0f, nullptr, 0, nullptr,
                           clip_probs, frame_probs);
    KCHK(a, "head");
    return LRCN_OK;
}

}  // extern "C"
