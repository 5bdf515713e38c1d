// lrcn_api.hip -- context, workspace and the C ABI of liblrcn_hip.so (include/lrcn.h).
//
// Orchestration of the hot path on one gfx950 device.  The reference runs lrcn() once per timestep with ~50 tiny
// kernels and a blocking D2H per step (lrcn.jl:560-570); here everything that does not feed back through the
// recurrence is time-batched over all S = T+1 steps (M = S*B rows, row m = s*B + b):
//   forward : embedding gather (+dropout) -> input-side gate GEMM for all steps -> S x [recurrent GEMM (beta=1) + fused
//             cell] -> projection GEMM -> concat/dropout -> LSTM-2 likewise -> ONE logits GEMM for all steps -> fused
//             log-softmax / NLL / dlogits with on-device double accumulation (no per-step D2H).
//   backward: dWout/dH2 GEMMs for all steps -> reverse recurrence (fused cell backward + one GEMM per step) ->
//             time-batched weight-gradient GEMMs (K = S*B) -> projection/x_cnn/embedding duals.
// Internal activations are row-major [row][feature] (K-contiguous) in the context's arithmetic type T (f32 or bf16);
// the column-major f32 arrays of the ABI are converted at the boundary.  Every contraction is the NT MFMA kernel of
// gemm.hip; operands that the math wants transposed are materialised K-contiguous by k_transpose.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "../../include/lrcn_varlen.h"
#include "../../include/lrcn_clip.h"

static thread_local std::string g_create_err;
using namespace lrcn_impl;

// Beside the capped convolution grids, from kBgMinRows rows, the large time-batched GEMMs walk their tiles persistently on this many
// workgroups per free CU instead of queueing hundreds: they get the same CUs either way, but take none from a convolution workgroup at a
// kernel boundary.
constexpr int kBgWgsPerFreeCu = 4;

// C[M][N] (+)= A[M][K] * B[N][K]^T
int lrcn_impl::gemm(lrcn_ctx *c, int dtype, const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc, int M, int N,
         int K, const float *bias, bool c_f32, bool beta, bool relu, bool c_is_zero, bool on_wg_stream) {
    GemmArgs g{};
    g.dtype = dtype;
    g.A = A;
    g.lda = lda;
    g.B = B;
    g.ldb = ldb;
    g.C = C;
    g.ldc = ldc;
    g.M = M;
    g.N = N;
    g.K = gemm_k(dtype, lda, ldb, K);
    g.bias = bias;
    g.c_f32 = c_f32;
    g.beta = beta;
    g.c_is_zero = c_is_zero;
    g.relu = relu;
    g.a_mode = GEMM_A_PLAIN;
    g.out_mode = GEMM_OUT_PLAIN;
    g.zero_page = c->zero_page;
    g.deterministic = c->opt_det;
    g.ws = on_wg_stream ? c->wg_ws : c->gemm_ws;  // one split-K workspace per stream
    g.ws_bytes = c->gemm_ws_bytes;
    if (!lstm_alone(c)) {  // beside the capped convolution grids: tell the router how many CUs those leave (gemm.h free_cus / bg_cus)
        const int free_cus = std::max(c->ncu - c->vgg_wg_cap, 0);
        if (c->cur_B < kBgMinRows) {
            g.free_cus = free_cus;
        } else {
            g.bg_cus = free_cus;
            if (free_cus >= 8) g.wg_cap = free_cus * kBgWgsPerFreeCu;
        }
    }
    hipError_t e = launch_gemm(on_wg_stream ? c->wg_stream : c->stream, g);
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "gemm M=%d N=%d K=%d: %s", M, N, K, hipGetErrorString(e));
    // kernel-development aid: LRCN_TRACE_ROUTES=1 prints which kernel family every contraction of a call took
    if (knob_char("LRCN_TRACE_ROUTES") == '1') {
        fprintf(stderr, "gemm M=%d N=%d K=%d %s-> %s\n", M, N, K, on_wg_stream ? "(wg stream) " : "", gemm_debug_last_route());
    }
    return LRCN_OK;
}

namespace {

DropSpec make_drop(const lrcn_dropout *d, int which) {
    DropSpec s{};
    s.which = which;
    if (d) {
        s.p = d->pdrop;
        s.seed = d->seed;
        s.mask = which == 1 ? d->mask1 : d->mask2;
        if (s.mask) s.p = 0.0f;
    }
    return s;
}

void ctx_sizes(const lrcn_ctx *c, int64_t sz[9]);
// the 14 training shadows as an array, in a fixed order (lrcn_ctx::alt mirrors it)
struct ShadowSet {
    void *W1x, *W1h, *W1xT, *W1hT, *W2x, *W2h, *W2xT, *W2hT, *Wpd, *WpT, *Wcd, *WeT, *Wod, *WoT;
};
ShadowSet cur_shadows(const lrcn_ctx *c) {
    return ShadowSet{c->W1x, c->W1h, c->W1xT, c->W1hT, c->W2x, c->W2h, c->W2xT, c->W2hT, c->Wpd, c->WpT, c->Wcd, c->WeT, c->Wod, c->WoT};
}
ShadowSet alt_shadows(const lrcn_ctx *c) {
    void *const *a = c->alt;
    return ShadowSet{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13]};
}
void swap_shadow_sets(lrcn_ctx *c) {
    void **cur[14] = {&c->W1x, &c->W1h, &c->W1xT, &c->W1hT, &c->W2x, &c->W2h, &c->W2xT, &c->W2hT, &c->Wpd, &c->WpT, &c->Wcd, &c->WeT, &c->Wod, &c->WoT};
    for (int i = 0; i < 14; ++i) std::swap(*cur[i], c->alt[i]);
    if (c->alt_gi[0]) {
        std::swap(c->W1h_gi, c->alt_gi[0]);
        std::swap(c->W2h_gi, c->alt_gi[1]);
    }
}
int ensure_alt_shadows(lrcn_ctx *c) {
    if (c->alt[0]) return LRCN_OK;
    const size_t es = c->esz;
    const int E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    const size_t bytes[14] = {es * 4 * H1 * c->ldX1, es * 4 * H1 * c->ldH1, es * X1 * c->ld4H1, es * H1 * c->ld4H1,
                              es * 4 * H2 * c->ldH2, es * 4 * H2 * c->ldH2, es * H2 * c->ld4H2, es * H2 * c->ld4H2,
                              es * h * c->ldH1, es * H1 * c->ldh, es * h * LRCN_CNNOUT, es * V * c->ldE, es * V * c->ldH2, es * H2 * c->ldV};
    (void)E;
    for (int i = 0; i < 14; ++i) DALLOC(c, c->alt[i], bytes[i]);  // zero-filled: the K padding must hold zeros
    return LRCN_OK;
}
// the gate-interleaved recurrent weights of BOTH sets (the cell-epilogue route of a training step under LRCN_OPT_FUSED_UPDATE)
int ensure_gi_sets(lrcn_ctx *c) {
    const bool two = c->nl == 2;
    if (!c->W1h_gi) DALLOC(c, c->W1h_gi, c->esz * 4 * c->H1 * c->ldH1);
    if (two && !c->W2h_gi) DALLOC(c, c->W2h_gi, c->esz * 4 * c->H2 * c->ldH2);
    if (c->opt_fused) {
        if (!c->alt_gi[0]) DALLOC(c, c->alt_gi[0], c->esz * 4 * c->H1 * c->ldH1);
        if (two && !c->alt_gi[1]) DALLOC(c, c->alt_gi[1], c->esz * 4 * c->H2 * c->ldH2);
    }
    return LRCN_OK;
}

// the six parameter matrices of the model -> descriptors of their shadows in `w` (memory images: see the comments per line)
void plan_matrices(const lrcn_ctx *c, const float *const p[9], const ShadowSet &w, bool b, PrepPlan &plan, int only_a = -1, int only_b = -1,
                   void *const *gi = nullptr) {   // gi: {W1h, W2h} destinations with (unit, gate)-interleaved rows, or NULL
    const int E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    const bool two = c->nl == 2;
    auto add = [&](int k, int R, int C, int cs, void *dA, int64_t ldA, void *dB, int64_t ldB, void *tA, int64_t ldtA, void *tB, int64_t ldtB) {
        if (only_a >= 0 && k != only_a && k != only_b) return;
        PrepDesc &d = plan.d[plan.n++];
        d = PrepDesc{};
        d.src = p[k]; d.R = R; d.C = C; d.cs = cs;
        d.dA = dA; d.ldA = ldA; d.dB = dB; d.ldB = ldB;
        d.tA = tA; d.ldtA = ldtA; d.tB = tB; d.ldtB = ldtB;
    };
    (void)E;
    // W1: memory [4H1][X1 + H1] -> W1x | W1h (and their transposes [X1][ld4H1] | [H1][ld4H1] for the backward dX GEMMs)
    auto with_gi = [&](int k, void *dst, int64_t ld, int H) {   // the descriptor just added (if `only` kept it) also writes the interleaved copy
        if (!dst || (only_a >= 0 && k != only_a && k != only_b)) return;
        PrepDesc &d = plan.d[plan.n - 1];
        d.dG = dst; d.ldG = ld; d.giH = H;
    };
    add(0, 4 * H1, X1 + H1, X1, w.W1x, c->ldX1, w.W1h, c->ldH1, b ? w.W1xT : nullptr, c->ld4H1, b ? w.W1hT : nullptr, c->ld4H1);
    with_gi(0, gi ? gi[0] : nullptr, c->ldH1, H1);
    if (two) {
        add(2, 4 * H2, 2 * H2, H2, w.W2x, c->ldH2, w.W2h, c->ldH2, b ? w.W2xT : nullptr, c->ld4H2, b ? w.W2hT : nullptr, c->ld4H2);
        with_gi(2, gi ? gi[1] : nullptr, c->ldH2, H2);
        add(4, h, H1, H1, w.Wpd, c->ldH1, nullptr, 0, b ? w.WpT : nullptr, c->ldh, nullptr, 0);  // Wproj (H1 x h): memory [h][H1]
    }
    add(5, h, LRCN_CNNOUT, LRCN_CNNOUT, w.Wcd, LRCN_CNNOUT, nullptr, 0, nullptr, 0, nullptr, 0);   // Wcnn: memory [h][4096]
    add(6, E, V, V, nullptr, 0, nullptr, 0, w.WeT, c->ldE, nullptr, 0);                          // Wembed (V x E): memory [E][V] -> [V][ldE]
    add(7, V, H2, H2, w.Wod, c->ldH2, nullptr, 0, b ? w.WoT : nullptr, c->ldV, nullptr, 0);   // Wout (H2 x V): memory [V][H2]
}

// the tensors of each gradient group, in the order of the grad_ev records in loss_impl
const int kGradGroup[LRCN_GRAD_GROUPS][2] = {{7, 8}, {2, 3}, {4, 5}, {0, 1}, {6, 6}};

// update! (lrcn.jl:394) of the tensors of gradient group `group` (-1: all nine) fused with the NEXT step's shadow pass (LRCN_OPT_FUSED_UPDATE):
// the kernel writes the not-current shadow set; the caller swaps the sets once every group has been issued.
int adam_fused(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group, int step, float lr,
               float b1, float b2, float eps, hipStream_t st, const ClipCtl *clip = nullptr) {
    int r = ensure_alt_shadows(c);
    if (r) return r;
    int64_t sz[9];
    ctx_sizes(c, sz);
    PrepPlan plan{};
    const int ka = group < 0 ? -1 : kGradGroup[group][0], kb = group < 0 ? -1 : kGradGroup[group][1];
    if (c->gi_live && (r = ensure_gi_sets(c))) return r;
    plan_matrices(c, p, alt_shadows(c), true, plan, ka, kb, c->gi_live ? c->alt_gi : nullptr);
    for (int i = 0; i < plan.n; ++i) {
        PrepDesc &d = plan.d[i];
        int k = 0;
        while (k < 9 && p[k] != d.src) ++k;
        d.g = g[k]; d.m = m[k]; d.v = v[k];
    }
    for (int k : {1, 3, 8}) {  // the biases: plain Adam, one "row" of n elements
        if (sz[k] == 0 || (group >= 0 && k != ka && k != kb)) continue;
        PrepDesc &d = plan.d[plan.n++];
        d = PrepDesc{};
        d.src = p[k]; d.g = g[k]; d.m = m[k]; d.v = v[k];
        d.R = 1; d.C = (int)sz[k]; d.cs = (int)sz[k];
    }
    // (a group's update on its own stream runs beside the rest of the backward pass on an UNCAPPED grid: the groups' updates are on the step's
    // critical path, not beside it)
    plan.clip = clip;  // non-NULL: the clipped form; a skipped step still writes this set, from the unchanged parameters
    k_adam_shadows(st, c->dt, plan, step, lr, b1, b2, eps);
    KCHK(c, "adam (fused with the shadow pass)");
    return LRCN_OK;
}
void fused_update_done(lrcn_ctx *c, float *const p[9]) {  // every tensor's Adam has been issued: the written set becomes the current one
    swap_shadow_sets(c);
    for (int k = 0; k < 9; ++k) c->shadow_p[k] = p[k];
    c->shadow_valid = true;
    c->shadow_has_gi = c->gi_live && c->alt_gi[0] != nullptr;
}

// The recurrent GEMM with the cell math in its epilogue (gemm_8p.hip GEMM_OUT_LSTM_*), for the two-stream training step at 256..512
// rows per GPU: one launch of 32 (forward) / 8 (backward) workgroups per timestep instead of GEMM + cell kernel.  LRCN_LSTM_EPI=f turns
// the forward one on, =1 both (tests/test_gpu_lstm_parity.py checks them against the CPU oracle).  OFF BY DEFAULT, with numbers:
//   round 2: one unit per epilogue thread -- per timestep beside the VGG forward, forward 45 us fused vs 27 + 9.6 us as two launches,
//            backward 87 us vs 55 + 8.7 us; training step 7.49 vs 7.22 ms.
//   round 6: the forward epilogue rewritten (four units per thread, c_prev / Gx requested before the staging, 16- / 8-byte accesses) and
//            its gate-interleaved weight copy kept current by the fused update: the forward recurrence's segment goes 1.00 -> 0.83 ms
//            per step (18.8 us per step and layer: FASTER than the two launches), and the training step does not move or gets slower:
//            five same-box pairs 6.858 -> 6.942 ms mean (profiles/r06_ab_c4_step_forward_cell_epilogue.txt), with the shader clock the
//            package holds in the timed region 2.163 -> 2.130 GHz median (bench line hw_held_in_timed_region) -- the convolution launches
//            beside it slow by what the chain gained, once more.  The backward epilogue stays at 8 workgroups (N = H:
//            eight 128-column tiles) and 1.94 vs 1.72 ms per step; a 32-workgroup form needs split-K, whose partial sums can only be
//            combined by a second launch or a grid barrier.
// The same forward epilogue IS the default of the batched beam decode (decode_gates_epi below), where its GEMMs fill the chip.
bool lstm_epi_on(lrcn_ctx *c, int B) {
    const char k = knob_char("LRCN_LSTM_EPI");
    return c->dt == GEMM_T_BF16 && !lstm_alone(c) && bg_row_window(B) && !(c->H1 & 3) && !(c->H2 & 3) && (k == '1' || k == 'f');
}
// LRCN_LSTM_EPI=f: the forward recurrence only (its launch has 32 workgroups -- one per free CU; the backward dh GEMM has N = H: 8 tiles)
bool lstm_epi_bwd_on(lrcn_ctx *c, int B, int H) {
    return lstm_epi_on(c, B) && knob_char("LRCN_LSTM_EPI") == '1' && H >= 128;   // its GEMM has N = H columns: at least one 128-column tile
}
// the recurrence's plain-form GEMM (host.h lstm_recurrence_*): gemm() on the context's stream, so the route hints of a step apply
auto rec_gemm(lrcn_ctx *c) {
    return [c](const void *A, int64_t lda, const void *B, int64_t ldb, float *C, int64_t ldc, int M, int N, int K, bool beta, bool c_is_zero) {
        return gemm(c, c->dt, A, lda, B, ldb, C, ldc, M, N, K, nullptr, true, beta, false, c_is_zero);
    };
}

// One LSTM layer over all S steps: the cell-epilogue route (lstm_epi_on, given the interleaved Wh_gi), else lstm_recurrence_fwd.
int lstm_layer_fwd(lrcn_ctx *c, int S, int B, int H, int64_t ldH, int64_t ld4H, float *Gx, const void *Wh, void *acts,
                   float *Call, void *Hall, const void *Wh_gi = nullptr) {
    const int dt = c->dt;
    const bool epi = !lstm_fused_on(dt, B, H, ldH, ld4H) && Wh_gi && lstm_epi_on(c, B);
    SegScope seg(c, LRCN_SEG_REC_FWD, c->stream, (double)(S - 1) * 4.0 * H * H * c->esz);  // one read of Wh (4H x H) per recurrent step
    if (!epi) {
        if (int r = lstm_recurrence_fwd(c, lstm_alone(c), rec_gemm(c), S, B, H, ldH, ld4H, Gx, Wh, acts, Call, Hall)) return r;
        KCHK(c, "lstm_layer_fwd");
        return LRCN_OK;
    }
    k_lstm_fwd(c->stream, dt, Gx, 4 * H, nullptr, B, H, acts, ld4H, Call, Hall, ldH, nullptr);
    for (int s = 1; s < S; ++s) {
        GemmArgs g{};
        g.dtype = dt;
        g.A = boff(Hall, (int64_t)(s - 1) * B * ldH, c->esz); g.lda = ldH;
        g.B = Wh_gi; g.ldb = ldH;
        g.M = B; g.N = 4 * H; g.K = (int)ldH;
        g.a_mode = GEMM_A_PLAIN;
        g.out_mode = GEMM_OUT_LSTM_FWD;
        g.zero_page = c->zero_page;
        g.lstm.H = H; g.lstm.ld_a = ld4H; g.lstm.ld_h = ldH;
        g.lstm.Gx = Gx + (int64_t)s * B * 4 * H;
        g.lstm.c_prev = Call + (int64_t)(s - 1) * B * H;
        g.lstm.c_out = Call + (int64_t)s * B * H;
        g.lstm.acts = boff(acts, (int64_t)s * B * ld4H, c->esz);
        g.lstm.h_new = boff(Hall, (int64_t)s * B * ldH, c->esz);
        hipError_t e = launch_gemm_8p(c->stream, g);
        if (e != hipSuccess) FAIL(c, LRCN_EHIP, "lstm fwd step (GEMM + cell epilogue): %s", hipGetErrorString(e));
    }
    KCHK(c, "lstm_layer_fwd");
    return LRCN_OK;
}

// Reverse recurrence of one layer: the cell-epilogue (lstm_epi_bwd_on) or K-sliced (LRCN_BWD_SLABS) route, else lstm_recurrence_bwd.
int lstm_layer_bwd(lrcn_ctx *c, int S, int B, int H, int64_t ld4H, const void *acts, const float *Call, const float *dHall,
                   const void *WhT, void *dZ) {
    const int dt = c->dt;
    const bool fused = lstm_fused_on(dt, B, H, ld64(H), ld4H);
    SegScope seg(c, LRCN_SEG_REC_BWD, c->stream, (double)(S - 1) * 4.0 * H * H * c->esz);
    if (!fused && lstm_epi_bwd_on(c, B, H)) {
        // cell backward of the last step, then one launch per step: dh_rec = dZ[s] Wh with the cell backward of s-1 in its epilogue
        k_lstm_bwd(c->stream, dt, boff(acts, (int64_t)(S - 1) * B * ld4H, c->esz), ld4H, S > 1 ? Call + (int64_t)(S - 2) * B * H : nullptr,
                   Call + (int64_t)(S - 1) * B * H, dHall + (int64_t)(S - 1) * B * H, H, nullptr, 0, c->dc, 1, B, H,
                   boff(dZ, (int64_t)(S - 1) * B * ld4H, c->esz), ld4H);
        for (int s = S - 1; s >= 1; --s) {
            GemmArgs g{};
            g.dtype = dt;
            g.A = boff(dZ, (int64_t)s * B * ld4H, c->esz); g.lda = ld4H;
            g.B = WhT; g.ldb = ld4H;
            g.M = B; g.N = H; g.K = (int)ld4H;
            g.a_mode = GEMM_A_PLAIN;
            g.out_mode = GEMM_OUT_LSTM_BWD;
            g.zero_page = c->zero_page;
            g.lstm.H = H; g.lstm.ld_a = ld4H;
            g.lstm.acts = const_cast<char *>(boff(acts, (int64_t)(s - 1) * B * ld4H, c->esz));
            g.lstm.c_prev = s > 1 ? Call + (int64_t)(s - 2) * B * H : nullptr;
            g.lstm.c_new = Call + (int64_t)(s - 1) * B * H;
            g.lstm.dh_ext = dHall + (int64_t)(s - 1) * B * H;
            g.lstm.dc = c->dc;
            g.lstm.dz_out = boff(dZ, (int64_t)(s - 1) * B * ld4H, c->esz);
            hipError_t e = launch_gemm_8p(c->stream, g);
            if (e != hipSuccess) FAIL(c, LRCN_EHIP, "lstm bwd step (GEMM + cell epilogue): %s", hipGetErrorString(e));
        }
        KCHK(c, "lstm_layer_bwd (epilogue)");
        return LRCN_OK;
    }
    // Beside the capped convolution grids at 256..512 rows the dh GEMM (M = B, N = H, K = 4H) has EIGHT 256 x 128 tiles: 8 of the 32 free CUs,
    // 3 MB of operand ingest each (55 us per timestep).  LRCN_BWD_SLABS=n (2..8; round 6): n K-slices per tile = 8 n workgroups, each writing
    // its partial tile to an f32 slab; the NEXT cell kernel sums the slabs (no reduce launch, fixed order: deterministic).  With n = 4, four
    // same-box pairs (profiles/r06_ab_bwd_slabs.txt): the backward recurrence's segment 1.86 -> 0.87 ms per step, the step 7.270 -> 7.241 ms
    // (-0.4 %: inside a lease's spread), the convolution launches beside the busier chain 0.571 -> 0.587 ms (+2.8 %, roofline.frac -0.013).
    // OFF BY DEFAULT like the forward cell epilogue: the LSTM chain is not what bounds the step, and a shorter chain is returned as a lower
    // clock for the convolutions; the route is kept, tested against the CPU oracle, for a configuration where the chain matters.
    {
        const int nsl = knob_int("LRCN_BWD_SLABS", 0);
        const int Kp = (int)round_up64(4 * H, 64);
        if (!fused && nsl >= 2 && nsl <= 8 && dt == GEMM_T_BF16 && !lstm_alone(c) && bg_row_window(B) && !(H & 3) && H >= 128 &&
            Kp / 64 >= 8 * nsl && Kp <= ld4H && (size_t)nsl * B * H * sizeof(float) <= c->gemm_ws_bytes && c->gemm_ws) {
            float *slabs = reinterpret_cast<float *>(c->gemm_ws);
            for (int s = S - 1; s >= 0; --s) {
                k_lstm_bwd(c->stream, dt, boff(acts, (int64_t)s * B * ld4H, c->esz), ld4H, s ? Call + (int64_t)(s - 1) * B * H : nullptr,
                           Call + (int64_t)s * B * H, dHall + (int64_t)s * B * H, H, slabs, s < S - 1, c->dc, s == S - 1, B, H,
                           boff(dZ, (int64_t)s * B * ld4H, c->esz), ld4H, nsl);
                if (s > 0) {
                    GemmArgs g{};
                    g.dtype = dt;
                    g.A = boff(dZ, (int64_t)s * B * ld4H, c->esz); g.lda = ld4H;
                    g.B = WhT; g.ldb = ld4H;
                    g.M = B; g.N = H; g.K = Kp;
                    g.C = slabs; g.ldc = H; g.c_f32 = 1;   // (unused: the slabs are the output)
                    g.a_mode = GEMM_A_PLAIN; g.out_mode = GEMM_OUT_PLAIN;
                    g.zero_page = c->zero_page;
                    g.ws = c->gemm_ws; g.ws_bytes = c->gemm_ws_bytes;
                    g.cfg_pref = 2;
                    g.splitk_forced = 1; g.splitk_no_reduce = 1;
                    hipError_t e = launch_gemm_8p(c->stream, g, nsl);
                    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "lstm bwd step (split-K slabs): %s", hipGetErrorString(e));
                }
            }
            KCHK(c, "lstm_layer_bwd (K slices summed by the cell kernel)");
            return LRCN_OK;
        }
    }
    if (int r = lstm_recurrence_bwd(c, lstm_alone(c), rec_gemm(c), S, B, H, ld4H, acts, Call, dHall, WhT, dZ)) return r;
    KCHK(c, fused ? "lstm_layer_bwd (fused)" : "lstm_layer_bwd");
    return LRCN_OK;
}

int check_shapes(lrcn_ctx *c, int T, int B, int norm_B) {
    if (T < 0 || T + 1 > c->maxS) FAIL(c, LRCN_EINVAL, "T=%d outside [0,%d]", T, c->maxS - 1);
    if (B < 1 || B > c->maxB) FAIL(c, LRCN_EINVAL, "B=%d outside [1,%d]", B, c->maxB);
    if (norm_B < 1) FAIL(c, LRCN_EINVAL, "norm_B=%d must be >= 1", norm_B);
    return LRCN_OK;
}

// lens (host, [B]) -> c->lens_dev on the context's stream, through the next pinned slot
int upload_lens(lrcn_ctx *c, const int32_t *lens, int B) {
    // each piece on its own guard: a call that failed half-way through here leaves the next one to create what is still missing
    if (!c->lens_dev) DALLOC(c, c->lens_dev, sizeof(int32_t) * (size_t)c->maxB);
    if (!c->lens_pin)
        HIPCHK(c, hipHostMalloc((void **)&c->lens_pin, sizeof(int32_t) * (size_t)c->maxB * lrcn_ctx::kLenSlots, hipHostMallocDefault));
    for (auto &e : c->lens_up)
        if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int k = c->lens_slot;
    c->lens_slot = (k + 1) % lrcn_ctx::kLenSlots;
    HIPCHK(c, hipEventSynchronize(c->lens_up[k]));  // returns at once for an event never recorded
    int32_t *slot = c->lens_pin + (size_t)k * c->maxB;
    std::memcpy(slot, lens, sizeof(int32_t) * (size_t)B);
    HIPCHK(c, hipMemcpyAsync(c->lens_dev, slot, sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->lens_up[k], c->stream));
    return LRCN_OK;
}

// loss / lossgradient on internal buffers. feats: B x 4096 column-major f32 (device).
// lens != NULL (host, [B]): the variable-length form of include/lrcn_varlen.h -- row b has lens[b] + 1 loss terms, the scale is
// 1 / norm_tokens and norm_B is not used.  Only the token builder and the softmax-NLL kernel differ; every launch in between is the same.
int loss_impl(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, int norm_B,
              const lrcn_dropout *drop, float *const grads[9], float *logits_out, const int32_t *lens = nullptr, int64_t norm_tokens = 0) {
    int r = check_shapes(c, T, B, norm_B);
    if (r) return r;
    if (lens) {
        if (norm_tokens < 1) FAIL(c, LRCN_EINVAL, "norm_tokens=%lld must be >= 1", (long long)norm_tokens);
        for (int b = 0; b < B; ++b)
            if (lens[b] < 0 || lens[b] > T) FAIL(c, LRCN_EINVAL, "lens[%d]=%d outside [0,%d]", b, lens[b], T);
    }
    if (drop && (drop->pdrop < 0.0f || drop->pdrop >= 1.0f)) FAIL(c, LRCN_EINVAL, "pdrop=%g outside [0,1)", drop->pdrop);
    if (drop && c->nl == 2 && ((drop->mask1 == nullptr) != (drop->mask2 == nullptr))) FAIL(c, LRCN_EINVAL, "mask1/mask2 must both be set");
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    const int S = T + 1, M = S * B;
    const size_t es = c->esz;
    hipStream_t st = c->stream;
    const bool bwd = grads != nullptr, two = c->nl == 2;
    if (bwd && (!grads[0] || !grads[1] || !grads[5] || !grads[6] || !grads[7] || !grads[8] || (two && (!grads[2] || !grads[3] || !grads[4]))))
        FAIL(c, LRCN_EINVAL, "null gradient tensor");
    const DropSpec d1 = make_drop(drop, 1), d2 = make_drop(drop, 2);
    const DropSpec none{};

    c->cur_B = B;
    const bool epi = lstm_epi_on(c, B) && !lstm_fused_on(c->dt, B, H1, c->ldH1, c->ld4H1);
    r = prepare_weights(c, p, bwd, false, epi);
    if (r) return r;
    if (lens) {
        if ((r = upload_lens(c, lens, B))) return r;
        k_build_tokens_var(st, tokens, c->lens_dev, T, B, V, c->tok_in, c->tok_tgt, c->logp);
    } else {
        k_build_tokens(st, tokens, T, B, V, c->tok_in, c->tok_tgt, c->logp);  // reads the caller's (T, B) ids once (T = 0: never)
    }
    // input = input * param[end-3]   lrcn.jl:558.  The two-layer model needs x_cnn only at LSTM-2's input, after the whole first
    // recurrence: its three launches (transpose, split-K GEMM, reduce: ~20 us at 32 rows) run on the weight-gradient stream beside that
    // chain and are joined before the concat (round 5).  Not beside the capped VGG forward from 256 rows (as the weight gradients:
    // there a second stream of LSTM-side workgroups takes CUs from the convolutions); LRCN_WG_STREAM=0 / 1 forces it off / on.
    const bool beside_vgg = !lstm_alone(c) && B >= kBgMinRows;
    const bool par = knob_set("LRCN_WG_STREAM") ? !knob_off("LRCN_WG_STREAM") : !beside_vgg;  // the weight-gradient stream is in use
    const bool xfork = two && par;
    auto image_embedding = [&](hipStream_t s_, bool on_wg) -> int {
        // feats (B x 4096 column-major = memory [4096][B]) -> F [B][4096] (T)
        k_transpose(s_, dt, 1, feats, B, LRCN_CNNOUT, B, c->F, LRCN_CNNOUT, 0);
        return gemm(c, dt, c->F, LRCN_CNNOUT, c->Wcd, LRCN_CNNOUT, c->xcnn, c->ldh, B, h, LRCN_CNNOUT, nullptr, true, false, false, false, on_wg);
    };
    int rx = LRCN_OK;
    if (xfork) {
        HIPCHK(c, hipEventRecord(c->xc_fork, st));
        HIPCHK(c, hipStreamWaitEvent(c->wg_stream, c->xc_fork, 0));
        rx = image_embedding(c->wg_stream, true);
        (void)hipEventRecord(c->xc_done, c->wg_stream);
    } else {
        rx = image_embedding(st, false);
        if (rx) return rx;
    }
    auto first_layer = [&]() -> int {
        // embeddings of [bos, tokens...] with the :542 dropout.  LRCN-1f: the LSTM input is dropout(hcat(embedding, x_cnn)) -- the
        // gather fills columns [0, E), the concat kernel appends x_cnn and applies the one mask over all E + h columns
        {
            SegScope seg(c, LRCN_SEG_EMBED_GATHER, st, 2.0 * M * E * es);  // (T+1) B rows of E elements read and written
            k_embed_gather(st, dt, c->WeT, c->ldE, c->tok_in, S, B, E, two ? d1 : none, c->Xemb, c->ldX1);
        }
        if (!two) k_concat_x2(st, dt, c->Xemb, c->ldX1, c->xcnn, c->ldh, S, B, E, h, d1);
        // LSTM 1
        GEMM(c, dt, c->Xemb, c->ldX1, c->W1x, c->ldX1, c->G1, 4 * H1, M, 4 * H1, X1, p[1], true);
        return lstm_layer_fwd(c, S, B, H1, c->ldH1, c->ld4H1, c->G1, c->W1h, c->A1, c->C1, c->H1all, epi ? c->W1h_gi : nullptr);
    };
    r = first_layer();
    if (xfork) {  // joined on EVERY exit: the side chain reads the caller's feats
        if (hipStreamWaitEvent(st, c->xc_done, 0) != hipSuccess) (void)hipStreamSynchronize(c->wg_stream);
        if (rx) return rx;
    }
    if (r) return r;
    const void *Htop = c->H1all;  // the hidden states the logits are computed from
    if (two) {
        // x = s[1]*w[end-4]; x = hcat(x, x_cnn); x = dropout(x)    lrcn.jl:544-547
        GEMM(c, dt, c->H1all, c->ldH1, c->Wpd, c->ldH1, c->X2, c->ldH2, M, h, H1, nullptr, false);
        k_concat_x2(st, dt, c->X2, c->ldH2, c->xcnn, c->ldh, S, B, h, h, d2);
        // LSTM 2
        GEMM(c, dt, c->X2, c->ldH2, c->W2x, c->ldH2, c->G2, 4 * H2, M, 4 * H2, H2, p[3], true);
        r = lstm_layer_fwd(c, S, B, H2, c->ldH2, c->ld4H2, c->G2, c->W2h, c->A2, c->C2, c->H2all, epi ? c->W2h_gi : nullptr);
        if (r) return r;
        Htop = c->H2all;
    }
    // logits for all steps: x * w[end-1] .+ w[end]   lrcn.jl:550
    GEMM(c, dt, Htop, c->ldH2, c->Wod, c->ldH2, c->Logits, c->ldV, M, V, H2, p[8], true);
    if (logits_out) {  // (T+1) blocks of B x V column-major: block s memory [V][B]
        for (int s = 0; s < S; ++s)
            k_transpose_f32(st, c->Logits + (int64_t)s * B * c->ldV, c->ldV, B, V, logits_out + (int64_t)s * B * V, B);
    }
    const float scale = (float)(1.0 / (lens ? (double)norm_tokens : (double)norm_B * (double)S));
    if (c->opt_det && !c->logp_rows) DALLOC(c, c->logp_rows, sizeof(double) * (size_t)c->maxS * c->maxB);
    (lens ? k_softmax_xent_masked : k_softmax_xent)(st, dt, c->Logits, c->ldV, c->tok_tgt, M, V, scale, c->logp, bwd ? c->dLog : nullptr, c->ldV,
                                                    c->opt_det ? c->logp_rows : nullptr);
    c->last_norm = norm_B;
    c->last_S = S;
    c->last_tokens = lens ? norm_tokens : 0;
    KCHK(c, "forward");
    if (!bwd) return LRCN_OK;

    const int64_t ldM = ld64(M), ldB = ld64(B);
    // Transposed operands of the weight-gradient GEMMs (contraction over the M = S*B rows) are materialised K-contiguous,
    // several per launch; the x- and h-side inputs of one LSTM share one stacked buffer so that dW = dZ' [x | h_prev] is
    // one GEMM per layer.
    auto tr = [&](TrPlan &pl, const void *src, int64_t ld_src, int R, int C, void *dst, int shift) {
        TrDesc &d = pl.d[pl.n++];
        d.src = src; d.ld_src = ld_src; d.R = R; d.C = C; d.dst = dst; d.ld_dst = ldM; d.shift = shift;
    };
    // The weight / bias gradients feed nothing but update!: they run on the context's weight-gradient stream (sw), forked from the
    // main chain by an event each time their operands are final, while the main stream goes on with the reverse recurrences --
    // chains of small launches that leave most CUs idle (alone on the chip) or some of the 32 free ones (beside the VGG forward).
    // Both streams only READ shared activations; TA / TB / dxcT / FT and the second split-K workspace belong to sw alone.
    // grad_ev[g] is recorded on whichever stream finalises group g; the main stream joins sw before the call returns.
    // Not from 256 rows per GPU beside the capped VGG forward: there the convolutions are the critical path and a second stream
    // of LSTM-side workgroups takes CUs from them at every kernel boundary (measured on one box, ms/step off -> on: LSTM step
    // alone 2.117 -> 2.052 at 256 rows, 1.086 -> 1.072 at 32; two-stream step 1.679 -> 1.611 at 32 but 7.38 -> 7.54 at 256).
    // LRCN_WG_STREAM=0 / 1 forces it off / on (`par`, above).
    hipStream_t sw = par ? c->wg_stream : st;
    int nfork = 0;
    auto fork = [&]() -> int {  // sw waits for everything issued on the main stream so far
        if (!par) return LRCN_OK;
        HIPCHK(c, hipEventRecord(c->wg_fork[nfork], st));
        HIPCHK(c, hipStreamWaitEvent(sw, c->wg_fork[nfork], 0));
        ++nfork;
        return LRCN_OK;
    };
#define FORK()                  \
    do {                        \
        int _r = fork();        \
        if (_r) return _r;      \
    } while (0)
    // Everything from the first fork on runs inside one scope whose every exit -- the normal one and each early error return --
    // is followed by the join below: an error after a fork must not leave the weight-gradient stream writing the caller's grads[]
    // (and reading the caller's feats) after the call has returned.
    auto backward = [&]() -> int {
    // ---- logits layer: dWout, dbout (sw) | dH2 (main) ----
        FORK();
        {
            TrPlan pl{};
            tr(pl, c->dLog, c->ldV, M, V, c->TA, 0);      // dLog^T [V][ldM]
            tr(pl, Htop, c->ldH2, M, H2, c->TB, 0);       // H2all^T [H2][ldM]
            k_transpose_multi(sw, dt, pl);
        }
        GEMM(c, dt, c->TA, ldM, c->TB, ldM, grads[7], H2, V, H2, M, nullptr, true, false, false, false, par);
        k_colsum(sw, dt, c->dLog, c->ldV, M, V, grads[8], c->opt_det);
        HIPCHK(c, hipEventRecord(c->grad_ev[0], sw));  // group 0: Wout, bout
        GEMM(c, dt, c->dLog, c->ldV, c->WoT, c->ldV, two ? c->dH2all : c->dH1all, H2, M, H2, V, nullptr, true);
        if (two) {
            // ---- LSTM 2 ----
            r = lstm_layer_bwd(c, S, B, H2, c->ld4H2, c->A2, c->C2, c->dH2all, c->W2hT, c->dZ2);
            if (r) return r;
            FORK();
            {
                TrPlan pl{};
                tr(pl, c->dZ2, c->ld4H2, M, 4 * H2, c->TA, 0);                              // dZ2^T [4H2][ldM]
                tr(pl, c->X2, c->ldH2, M, H2, c->TB, 0);                                     // X2^T [2h][ldM]
                tr(pl, c->H2all, c->ldH2, M - B, H2, boff(c->TB, (int64_t)H2 * ldM, es), M > B ? B : 0);  // h2_prev^T (one step later)
                k_transpose_multi(sw, dt, pl);
            }
            GEMM(c, dt, c->TA, ldM, c->TB, ldM, grads[2], 2 * H2, 4 * H2, 2 * H2, M, nullptr, true, false, false, false, par);
            k_colsum(sw, dt, c->dZ2, c->ld4H2, M, 4 * H2, grads[3], c->opt_det);
        }
        HIPCHK(c, hipEventRecord(c->grad_ev[1], sw));  // group 1: W2, b2
        if (two) {
            GEMM(c, dt, c->dZ2, c->ld4H2, c->W2xT, c->ld4H2, c->dX2, c->ldH2, M, H2, 4 * H2, nullptr, false);
            k_dx2_mask_reduce(st, dt, c->dX2, c->ldH2, S, B, h, h, d2, c->dxcnn, c->ldh);
            // ---- projection and image embedding: dWproj, dWcnn (sw) | dH1 (main) ----
            FORK();
            {
                TrPlan pl{};
                tr(pl, c->dX2, c->ldH2, M, h, c->TA, 0);      // dP^T [h][ldM]
                tr(pl, c->H1all, c->ldH1, M, H1, c->TB, 0);   // H1all^T [H1][ldM]
                k_transpose_multi(sw, dt, pl);
            }
            GEMM(c, dt, c->TA, ldM, c->TB, ldM, grads[4], H1, h, H1, M, nullptr, true, false, false, false, par);
            GEMM(c, dt, c->dX2, c->ldH2, c->WpT, c->ldh, c->dH1all, H1, M, H1, h, nullptr, true);
            k_transpose(sw, dt, 1, c->dxcnn, c->ldh, B, h, c->dxcT, ldB, 0);     // dxcnn^T [h][ldB]
            k_cast_rows(sw, dt, feats, B, LRCN_CNNOUT, B, c->FT, ldB);           // feats^T [4096][ldB] (it already is, in memory)
            GEMM(c, dt, c->dxcT, ldB, c->FT, ldB, grads[5], LRCN_CNNOUT, h, LRCN_CNNOUT, B, nullptr, true, false, false, false, par);
            HIPCHK(c, hipEventRecord(c->grad_ev[2], sw));  // group 2: Wproj, Wcnn
        }
        // ---- LSTM 1 ----
        r = lstm_layer_bwd(c, S, B, H1, c->ld4H1, c->A1, c->C1, c->dH1all, c->W1hT, c->dZ1);
        if (r) return r;
        FORK();
        {
            TrPlan pl{};
            tr(pl, c->dZ1, c->ld4H1, M, 4 * H1, c->TA, 0);
            tr(pl, c->Xemb, c->ldX1, M, X1, c->TB, 0);
            tr(pl, c->H1all, c->ldH1, M - B, H1, boff(c->TB, (int64_t)X1 * ldM, es), M > B ? B : 0);
            k_transpose_multi(sw, dt, pl);
        }
        GEMM(c, dt, c->TA, ldM, c->TB, ldM, grads[0], X1 + H1, 4 * H1, X1 + H1, M, nullptr, true, false, false, false, par);
        k_colsum(sw, dt, c->dZ1, c->ld4H1, M, 4 * H1, grads[1], c->opt_det);
        HIPCHK(c, hipEventRecord(c->grad_ev[3], sw));  // group 3: W1, b1
        GEMM(c, dt, c->dZ1, c->ld4H1, c->W1xT, c->ld4H1, c->dXemb, c->ldX1, M, X1, 4 * H1, nullptr, true);
        if (!two) {
            // LRCN-1f: d[embedding | x_cnn] -- mask all E + h columns in place, sum the right h columns over the steps -> d x_cnn,
            // then the image-embedding gradient exactly as in the two-layer model (on sw, after the dW1 GEMM that shares its scratch)
            k_dx2_mask_reduce(st, GEMM_T_F32, c->dXemb, c->ldX1, S, B, E, h, d1, c->dxcnn, c->ldh);
            FORK();
            k_transpose(sw, dt, 1, c->dxcnn, c->ldh, B, h, c->dxcT, ldB, 0);
            k_cast_rows(sw, dt, feats, B, LRCN_CNNOUT, B, c->FT, ldB);
            GEMM(c, dt, c->dxcT, ldB, c->FT, ldB, grads[5], LRCN_CNNOUT, h, LRCN_CNNOUT, B, nullptr, true, false, false, false, par);
            HIPCHK(c, hipEventRecord(c->grad_ev[2], sw));  // group 2: Wcnn
        }
        SegScope seg_eg(c, LRCN_SEG_EMBED_GRAD, st, 4.0 * M * E + 4.0 * (double)V * E);  // (T+1) B rows of E f32 in, dense V x E f32 out
        if (c->emb_rows_out) {
            // data-parallel host with the sparse exchange on: hand out this rank's rows and ids; grads[6] is NOT written by this call
            if (M > c->emb_rows_cap) FAIL(c, LRCN_EINVAL, "embedding-row buffer holds %d rows, this call has %d", c->emb_rows_cap, M);
            k_embed_rows_export(st, c->dXemb, c->ldX1, S, B, E, two ? d1 : none, c->emb_rows_out);
            HIPCHK(c, hipMemcpyAsync(c->emb_tok_out, c->tok_in, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToDevice, st));
        } else {
            // dWembed: per-token sums in an E-contiguous staging array, then one transpose into the column-major gradient (train_kernels.hip).
            if (!c->dWe_rm) DALLOC(c, c->dWe_rm, sizeof(float) * (size_t)V * c->ldE);
            unsigned long long *keys = nullptr;
            if (c->opt_det) {
                if (!c->sort_keys) DALLOC(c, c->sort_keys, sizeof(unsigned long long) * (size_t)c->maxS * c->maxB);
                keys = c->sort_keys;
            }
            // declines only with sort keys: more rows than the counting sort ranks
            if (!k_embed_scatter_rm(st, c->dXemb, c->ldX1, c->tok_in, S, B, E, V, two ? d1 : none, c->dWe_rm, c->ldE, grads[6], keys))
                FAIL(c, LRCN_EINVAL, "LRCN_OPT_DETERMINISTIC supports (T+1)*B <= 8192 rows per call (got %d)", M);
        }
        HIPCHK(c, hipEventRecord(c->grad_ev[4], st));  // group 4: Wembed
        return LRCN_OK;
    };
    r = backward();
    if (par && nfork > 0) {  // join: whatever follows on the main stream (update!, the next call's scratch reuse) comes after the weight gradients
        const hipError_t e1 = hipEventRecord(c->wg_done, sw);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(st, c->wg_done, 0) : e1;
        if (e2 != hipSuccess) {
            (void)hipStreamSynchronize(sw);  // the event path failed: fall back to a host-side join rather than return unjoined
            if (!r) FAIL(c, LRCN_EHIP, "joining the weight-gradient stream: %s", hipGetErrorString(e2));
        }
    }
    if (r) return r;
#undef FORK
    KCHK(c, "backward");
    return LRCN_OK;
}

// logp[0] = running sum of log p(target); logp[1] = sticky "token id outside [0, V)" flag raised by build_tokens_kernel
int fetch_loss(lrcn_ctx *c, double *out) {
    double s[2] = {0.0, 0.0};
    HIPCHK(c, hipMemcpyAsync(s, c->logp, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (s[1] != 0.0) {
        HIPCHK(c, hipMemsetAsync(c->logp + 1, 0, sizeof(double), c->stream));
        FAIL(c, LRCN_EINVAL, "a token id was outside [0, V=%d) (ids are 0-based at the ABI: eos=0, bos=1, unk=2; the reference raises BoundsError, lrcn.jl:556/569)", c->V);
    }
    if (out) *out = -s[0] / (c->last_tokens > 0 ? (double)c->last_tokens : (double)c->last_norm * (double)c->last_S);
    return LRCN_OK;
}

// element counts of the context's 9 tensors (0 for the slots its model does not have)
void ctx_sizes(const lrcn_ctx *c, int64_t sz[9]) { lrcn_param_sizes_n(c->nl, c->E, c->H1, c->H2, c->V, sz); }

// ------------------------------------------------------------------------------------------- data parallelism

// LRCN_DP_FORCE_PIPELINE=1: run the per-group [all-reduce -> Adam] pipeline (and the collectives) even on a one-rank communicator,
// so that a single-GPU box exercises exactly the code N > 1 runs (tests)
bool dp_force_pipeline() {
    return knob_char("LRCN_DP_FORCE_PIPELINE") == '1';
}

int ensure_buckets(lrcn_ctx *c) {
    if (!c->comm_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
        c->comm_stream_owned = true;
    }
    for (int g = 0; g < LRCN_GRAD_GROUPS; ++g) {
        c->bucket[g] = c->comm_stream;
        if (!c->bucket_done[g]) HIPCHK(c, hipEventCreateWithFlags(&c->bucket_done[g], hipEventDisableTiming));
        if (!c->ar_done[g]) HIPCHK(c, hipEventCreateWithFlags(&c->ar_done[g], hipEventDisableTiming));
    }
    return LRCN_OK;
}

// The communicator's stream waits for the group's gradient-ready event and all-reduces the group's tensors in place (one collective
// when they are adjacent in memory, which they are in a flat gradient buffer); the group's own stream -- on which the caller may
// queue that group's Adam -- waits for the collective.  One stream for all collectives: the same issue order on every rank, no
// concurrent use of one communicator from several streams.
int allreduce_group(lrcn_ctx *c, float *const grads[9], int group) {
    int64_t sz[9];
    ctx_sizes(c, sz);
    hipStream_t s = c->comm_stream;
    HIPCHK(c, hipStreamWaitEvent(s, c->grad_ev[group], 0));
    if (c->comm && (comm_world(c->comm) > 1 || dp_force_pipeline())) {
        char err[256] = "";
        const int k0 = kGradGroup[group][0], k1 = kGradGroup[group][1];
        int rc = 0;
        if (k0 == k1 || sz[k1] == 0) {
            rc = comm_allreduce_f32(c->comm, grads[k0], (size_t)sz[k0], s, err, sizeof(err));
        } else if (sz[k0] == 0) {
            rc = comm_allreduce_f32(c->comm, grads[k1], (size_t)sz[k1], s, err, sizeof(err));
        } else if (grads[k0] + sz[k0] == grads[k1]) {
            rc = comm_allreduce_f32(c->comm, grads[k0], (size_t)(sz[k0] + sz[k1]), s, err, sizeof(err));
        } else {
            comm_group_begin(c->comm);
            rc = comm_allreduce_f32(c->comm, grads[k0], (size_t)sz[k0], s, err, sizeof(err));
            if (!rc) rc = comm_allreduce_f32(c->comm, grads[k1], (size_t)sz[k1], s, err, sizeof(err));
            comm_group_end(c->comm);
        }
        if (rc) FAIL(c, LRCN_EHIP, "%s", err);
    }
    HIPCHK(c, hipEventRecord(c->ar_done[group], s));
    HIPCHK(c, hipStreamWaitEvent(c->bucket[group], c->ar_done[group], 0));
    c->bucket_pending[group] = true;
    return LRCN_OK;
}

int join_buckets(lrcn_ctx *c) {
    for (int g = 0; g < LRCN_GRAD_GROUPS; ++g)
        if (c->bucket_pending[g]) {
            HIPCHK(c, hipEventRecord(c->bucket_done[g], c->bucket[g]));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->bucket_done[g], 0));
            c->bucket_pending[g] = false;
        }
    return LRCN_OK;
}

}  // namespace

// f32 column-major params -> K-contiguous shadows in T (direct and transposed).  See DESIGN.md "shadow weights".
int lrcn_impl::prepare_weights(lrcn_ctx *c, const float *const p[9], bool need_bwd, bool cat, bool gi, bool cat_perm,
                    bool dec_tables) {   // dec_tables: the interleaved recurrent copies + W2 without its x_cnn columns (a decode call: not sticky)
    const int dt = c->dt, H1 = c->H1, H2 = c->H2, X1 = c->X1;
    if (!p[0] || !p[1] || !p[5] || !p[6] || !p[7] || !p[8] || (c->nl == 2 && (!p[2] || !p[3] || !p[4]))) FAIL(c, LRCN_EINVAL, "null parameter tensor");
    hipStream_t st = c->stream;
    const bool two = c->nl == 2;
    // LRCN_OPT_FUSED_UPDATE: the previous train step's Adam kernel already wrote this set from these very parameters
    if (gi || dec_tables) {
        int rg = ensure_gi_sets(c);
        if (rg) return rg;
        if (gi) c->gi_live = true;   // from now on the fused update writes the interleaved copies with the other shadows
    }
    if (dec_tables) gi = true;
    if (c->opt_fused && c->shadow_valid && !cat && (!gi || c->shadow_has_gi)) {
        bool same = true;
        for (int k = 0; k < 9; ++k) same = same && c->shadow_p[k] == p[k];
        if (same) return LRCN_OK;
    }
    c->shadow_valid = false;
    c->refresh_groups = 0;  // a full shadow pass supersedes a per-group refresh sequence that was left unfinished
    PrepPlan plan{};
    void *const gi_cur[2] = {c->W1h_gi, c->W2h_gi};
    plan_matrices(c, p, cur_shadows(c), need_bwd, plan, -1, -1, gi ? gi_cur : nullptr);
    if (dec_tables && c->nl == 2) {
        // W2 (memory [4H2][2 H2]: columns [h1 Wproj (h) | x_cnn (h) | h2 (H2)]) -> dec_W2c [4H2][ldh + ldH2] = [proj columns | h2 columns], rows
        // (unit, gate)-interleaved: two descriptors over the same source, each with one live side
        const int64_t ld = c->ldh + c->ldH2;
        PrepDesc &a = plan.d[plan.n++];
        a = PrepDesc{};
        a.src = p[2]; a.R = 4 * H2; a.C = 2 * H2; a.cs = c->h; a.dA = c->dec_W2c; a.ldA = ld; a.permH = H2;
        PrepDesc &b = plan.d[plan.n++];
        b = PrepDesc{};
        b.src = p[2]; b.R = 4 * H2; b.C = 2 * H2; b.cs = H2; b.dB = boff(c->dec_W2c, c->ldh, c->esz); b.ldB = ld; b.permH = H2;
    }
    if (cat) {  // batched decode: W1 / W2 with the x and h column blocks each padded to whole K-steps, side by side
        // cat_perm: the rows in (unit, gate)-interleaved order, for the decode step with the cell math in the GEMM's epilogue
        auto add = [&](const float *src, int R, int C, int cs, void *dA, int64_t ldA, void *dB, int64_t ldB, int permH) {
            PrepDesc &d = plan.d[plan.n++];
            d = PrepDesc{};
            d.src = src; d.R = R; d.C = C; d.cs = cs; d.dA = dA; d.ldA = ldA; d.dB = dB; d.ldB = ldB;
            d.permH = cat_perm ? permH : 0;
        };
        add(p[0], 4 * H1, X1 + H1, X1, c->W1cat, c->ldXH1, boff(c->W1cat, c->ldX1, c->esz), c->ldXH1, H1);
        if (two) add(p[2], 4 * H2, 2 * H2, H2, c->W2cat, c->ldXH2, boff(c->W2cat, c->ldH2, c->esz), c->ldXH2, H2);
    }
    k_prepare_weights(st, dt, plan);
    KCHK(c, "prepare_weights");
    return LRCN_OK;
}

// lrcn() on internal single-step buffers: state st_f32 (f32 row-major), inputs st_x (T [B][ldX1]: the embedding in columns
// [0, E); LRCN-1f appends x_cnn here) and xcnn (f32 [B][ldh]).
// d2: dropout of the concatenated input (LSTM-2's in the two-layer model, LSTM-1's in LRCN-1f). Leaves logits in st_logits [B][ldV].
int lrcn_impl::step_internal(lrcn_ctx *c, const float *const p[9], int B, const DropSpec &d2, bool h_ready) {
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    hipStream_t st = c->stream;
    const bool two = c->nl == 2;
    if (!two) k_concat_x2(st, dt, c->st_x, c->ldX1, c->xcnn, c->ldh, 1, B, E, h, d2);  // x = dropout(hcat(x_lstm, x_cnn))
    // LSTM 1: gates = x*W1x' + h1*W1h' + b1
    if (!h_ready) k_cast_rows(st, dt, c->st_f32[0], H1, B, H1, c->st_h1, c->ldH1);  // h_ready: st_h1 / st_h2 already hold T(h)
    GEMM(c, dt, c->st_x, c->ldX1, c->W1x, c->ldX1, c->st_g, 4 * H1, B, 4 * H1, X1, p[1], true);
    GEMM(c, dt, c->st_h1, c->ldH1, c->W1h, c->ldH1, c->st_g, 4 * H1, B, 4 * H1, H1, nullptr, true, true);
    k_lstm_fwd(st, dt, c->st_g, 4 * H1, c->st_f32[1], B, H1, c->st_a, c->ld4H1, c->st_f32[1], c->st_h1, c->ldH1, c->st_f32[0]);
    if (!two) {
        GEMM(c, dt, c->st_h1, c->ldH1, c->Wod, c->ldH2, c->st_logits, c->ldV, B, V, H2, p[8], true);
        KCHK(c, "step (1 layer)");
        return LRCN_OK;
    }
    // projection + concat + dropout
    GEMM(c, dt, c->st_h1, c->ldH1, c->Wpd, c->ldH1, c->st_x2, c->ldH2, B, h, H1, nullptr, false);
    k_concat_x2(st, dt, c->st_x2, c->ldH2, c->xcnn, c->ldh, 1, B, h, h, d2);
    // LSTM 2
    if (!h_ready) k_cast_rows(st, dt, c->st_f32[2], H2, B, H2, c->st_h2, c->ldH2);
    GEMM(c, dt, c->st_x2, c->ldH2, c->W2x, c->ldH2, c->st_g, 4 * H2, B, 4 * H2, H2, p[3], true);
    GEMM(c, dt, c->st_h2, c->ldH2, c->W2h, c->ldH2, c->st_g, 4 * H2, B, 4 * H2, H2, nullptr, true, true);
    k_lstm_fwd(st, dt, c->st_g, 4 * H2, c->st_f32[3], B, H2, c->st_a, c->ld4H2, c->st_f32[3], c->st_h2, c->ldH2, c->st_f32[2]);
    GEMM(c, dt, c->st_h2, c->ldH2, c->Wod, c->ldH2, c->st_logits, c->ldV, B, V, H2, p[8], true);
    KCHK(c, "step");
    return LRCN_OK;
}

// =====================================================================================================
extern "C" {

const char *lrcn_version(void) { return "lrcn-hip 0.4 (gfx950)"; }
int lrcn_abi_version(void) { return LRCN_ABI_VERSION; }

int lrcn_set_option(lrcn_ctx *c, int option, int64_t value) {
    if (!c) return LRCN_EINVAL;
    switch (option) {
    case LRCN_OPT_FUSED_UPDATE:
        if (value != 0 && value != 1) FAIL(c, LRCN_EINVAL, "LRCN_OPT_FUSED_UPDATE takes 0 or 1");
        c->opt_fused = value != 0;
        c->shadow_valid = false;
        c->fused_groups = 0;
        if (c->opt_fused) {  // the second shadow set is allocated here, not inside the first update (no allocation in a step)
            DeviceGuard dg(c);
            return ensure_alt_shadows(c);
        }
        return LRCN_OK;
    case LRCN_OPT_DETERMINISTIC:
        if (value != 0 && value != 1) FAIL(c, LRCN_EINVAL, "LRCN_OPT_DETERMINISTIC takes 0 or 1");
        c->opt_det = value != 0;
        return LRCN_OK;
    case LRCN_OPT_CONV_CHUNK_BYTES:
        if (value < 0) FAIL(c, LRCN_EINVAL, "LRCN_OPT_CONV_CHUNK_BYTES must be >= 0");
        c->conv_chunk_bytes = value;
        return LRCN_OK;
    default:
        FAIL(c, LRCN_EINVAL, "unknown option %d", option);
    }
}

int lrcn_params_touched(lrcn_ctx *c) {
    if (!c) return LRCN_EINVAL;
    c->shadow_valid = false;
    c->fused_groups = 0;  // a per-group update that stopped partway must not complete a later step's mask
    c->refresh_groups = 0;
    return LRCN_OK;
}

const char *lrcn_last_error(const lrcn_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int lrcn_param_sizes_n(int n_layers, int E, int H1, int H2, int V, int64_t s[9]) {
    if (E < 1 || H1 < 1 || H2 < 2 || (H2 & 1) || V < 3 || !s) return LRCN_EINVAL;
    if (n_layers != 0 && n_layers != 1 && n_layers != 2) return LRCN_EINVAL;
    const int h = H2 / 2;
    if (n_layers == 1) {  // LRCN-1f: one LSTM over [embedding | x_cnn]; W2, b2, Wproj do not exist
        if (H1 != H2) return LRCN_EINVAL;
        s[0] = (int64_t)(E + h + H1) * 4 * H1;
        s[2] = s[3] = s[4] = 0;
    } else {
        s[0] = (int64_t)(E + H1) * 4 * H1;
        s[2] = (int64_t)(2 * H2) * 4 * H2;
        s[3] = 4 * H2;
        s[4] = (int64_t)H1 * h;
    }
    s[1] = 4 * H1;
    s[5] = (int64_t)LRCN_CNNOUT * h;
    s[6] = (int64_t)V * E;
    s[7] = (int64_t)H2 * V;
    s[8] = V;
    return LRCN_OK;
}
int lrcn_param_sizes(int E, int H1, int H2, int V, int64_t s[9]) { return lrcn_param_sizes_n(2, E, H1, H2, V, s); }

int lrcn_malloc(void **p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 16) == hipSuccess ? LRCN_OK : LRCN_ENOMEM; }
int lrcn_free(void *p) { return hipFree(p) == hipSuccess ? LRCN_OK : LRCN_EHIP; }
int lrcn_memcpy_h2d(void *d, const void *s, size_t n) { return hipMemcpy(d, s, n, hipMemcpyHostToDevice) == hipSuccess ? LRCN_OK : LRCN_EHIP; }
int lrcn_memcpy_d2h(void *d, const void *s, size_t n) { return hipMemcpy(d, s, n, hipMemcpyDeviceToHost) == hipSuccess ? LRCN_OK : LRCN_EHIP; }

void lrcn_destroy(lrcn_ctx *c) {
    if (!c) return;
    DeviceGuard dg(c);
    (void)hipDeviceSynchronize();
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->sc_arena) (void)hipFree(c->sc_arena);
    for (auto &e : c->grad_ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->wg_fork)
        if (e) (void)hipEventDestroy(e);
    if (c->wg_done) (void)hipEventDestroy(c->wg_done);
    if (c->xc_fork) (void)hipEventDestroy(c->xc_fork);
    if (c->xc_done) (void)hipEventDestroy(c->xc_done);
    if (c->pin) (void)hipHostFree(c->pin);
    if (c->lens_pin) (void)hipHostFree(c->lens_pin);
    for (auto &e : c->lens_up)
        if (e) (void)hipEventDestroy(e);
    if (c->wg_stream && c->wg_stream_owned) (void)hipStreamDestroy(c->wg_stream);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (int j = 0; j < lrcn_ctx::kStage; ++j) {
        if (c->up_done[j]) (void)hipEventDestroy(c->up_done[j]);
        if (c->rd_done[j]) (void)hipEventDestroy(c->rd_done[j]);
    }
    comm_destroy(c->comm);
    for (auto &e : c->bucket_done)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->ar_done)
        if (e) (void)hipEventDestroy(e);
    if (c->comm_stream && c->comm_stream_owned) (void)hipStreamDestroy(c->comm_stream);
    for (auto &sp : c->seg)
        for (auto &e : sp.ev) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    for (auto &e : c->prof_ev) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    delete c;
}

int lrcn_create(const lrcn_config *cfg, lrcn_ctx **out) {
    if (!cfg || !out) {
        g_create_err = "null argument";
        return LRCN_EINVAL;
    }
    *out = nullptr;
    int64_t sz[9];
    if (lrcn_param_sizes_n(cfg->n_layers, cfg->E, cfg->H1, cfg->H2, cfg->V, sz) != LRCN_OK || cfg->max_B < 1 || cfg->max_T < 0 ||
        cfg->max_T > LRCN_MAX_T || (cfg->lstm_dtype != LRCN_F32 && cfg->lstm_dtype != LRCN_BF16) ||
        (cfg->vgg_dtype != LRCN_F32 && cfg->vgg_dtype != LRCN_BF16 && cfg->vgg_dtype != LRCN_FP8) || cfg->max_images < 0) {
        g_create_err = "invalid lrcn_config (need E,H1>=1, even H2>=2, V>=3, max_B>=1, 0<=max_T<=28, lstm_dtype in {F32,BF16}, vgg_dtype in {F32,BF16,FP8}, n_layers in {0,1,2} with H1 == H2 when n_layers == 1)";
        return LRCN_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev) {
        g_create_err = "no such HIP device (is a GPU visible?)";
        return LRCN_EHIP;
    }
    lrcn_ctx *c = new lrcn_ctx();
    c->cfg = *cfg;
    DeviceGuard dg(c);  // allocate on cfg->device, then restore the caller's selection
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != cfg->device) {
            g_create_err = "hipSetDevice failed";
            delete c;
            return LRCN_EHIP;
        }
    }
    c->opt_det = knob_char("LRCN_DETERMINISTIC") == '1';  // environment default of the option (lrcn_set_option overrides)
    if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess || c->ncu < 1) c->ncu = 256;
    c->dt = cfg->lstm_dtype == LRCN_BF16 ? GEMM_T_BF16 : GEMM_T_F32;
    c->vdt = cfg->vgg_dtype == LRCN_F32 ? GEMM_T_F32 : GEMM_T_BF16;  // LRCN_FP8: bf16 everywhere outside conv2_2..conv5_3
    c->vgg_fp8 = cfg->vgg_dtype == LRCN_FP8;
    c->esz = c->dt == GEMM_T_BF16 ? 2 : 4;
    c->vesz = c->vdt == GEMM_T_BF16 ? 2 : 4;
    c->E = cfg->E; c->H1 = cfg->H1; c->H2 = cfg->H2; c->h = cfg->H2 / 2; c->V = cfg->V;
    c->nl = cfg->n_layers == 1 ? 1 : 2;
    c->X1 = c->nl == 1 ? c->E + c->h : c->E;
    c->maxB = cfg->max_B; c->maxS = cfg->max_T + 1;
    const int E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, B = c->maxB, S = c->maxS;
    const int64_t M = (int64_t)S * B;
    const int X1 = c->X1;
    c->ldX1 = ld64(X1);
    c->ldE = ld64(E); c->ldH1 = ld64(H1); c->ldH2 = ld64(H2); c->ldh = ld64(h); c->ld4H1 = ld64(4 * H1); c->ld4H2 = ld64(4 * H2);
    c->ldV = ld64(V); c->ldM = ld64(M); c->ldB = ld64(B);
    const size_t es = c->esz;
    int rc = [&]() -> int {
        c->ldXH1 = c->ldX1 + c->ldH1; c->ldXH2 = 2 * c->ldH2;
        DALLOC(c, c->W1cat, es * 4 * H1 * c->ldXH1); DALLOC(c, c->W2cat, es * 4 * H2 * c->ldXH2);
        DALLOC(c, c->st_xh1, es * B * c->ldXH1);     DALLOC(c, c->st_xh2, es * B * c->ldXH2);
        DALLOC(c, c->W1x, es * 4 * H1 * c->ldX1);  DALLOC(c, c->W1h, es * 4 * H1 * c->ldH1);
        DALLOC(c, c->W1xT, es * X1 * c->ld4H1);    DALLOC(c, c->W1hT, es * H1 * c->ld4H1);
        DALLOC(c, c->W2x, es * 4 * H2 * c->ldH2);  DALLOC(c, c->W2h, es * 4 * H2 * c->ldH2);
        DALLOC(c, c->W2xT, es * H2 * c->ld4H2);    DALLOC(c, c->W2hT, es * H2 * c->ld4H2);
        DALLOC(c, c->Wpd, es * h * c->ldH1);       DALLOC(c, c->WpT, es * H1 * c->ldh);
        DALLOC(c, c->Wcd, es * h * LRCN_CNNOUT);   DALLOC(c, c->WeT, es * V * c->ldE);
        DALLOC(c, c->Wod, es * V * c->ldH2);       DALLOC(c, c->WoT, es * H2 * c->ldV);
        DALLOC(c, c->tok, sizeof(int32_t) * M);    DALLOC(c, c->tok_in, sizeof(int32_t) * M);
        DALLOC(c, c->tok_tgt, sizeof(int32_t) * M);
        DALLOC(c, c->F, es * B * LRCN_CNNOUT);     DALLOC(c, c->FT, es * LRCN_CNNOUT * c->ldB);
        DALLOC(c, c->xcnn, sizeof(float) * B * c->ldh);
        DALLOC(c, c->Xemb, es * M * c->ldX1);
        DALLOC(c, c->G1, sizeof(float) * M * 4 * H1); DALLOC(c, c->A1, es * M * c->ld4H1);
        DALLOC(c, c->C1, sizeof(float) * M * H1);     DALLOC(c, c->H1all, es * M * c->ldH1);
        DALLOC(c, c->X2, es * M * c->ldH2);
        DALLOC(c, c->G2, sizeof(float) * M * 4 * H2); DALLOC(c, c->A2, es * M * c->ld4H2);
        DALLOC(c, c->C2, sizeof(float) * M * H2);     DALLOC(c, c->H2all, es * M * c->ldH2);
        DALLOC(c, c->Logits, sizeof(float) * M * c->ldV);
        DALLOC(c, c->dLog, es * M * c->ldV);
        DALLOC(c, c->dZ1, es * M * c->ld4H1);      DALLOC(c, c->dZ2, es * M * c->ld4H2);
        DALLOC(c, c->dX2, es * M * c->ldH2);
        DALLOC(c, c->dH1all, sizeof(float) * M * H1); DALLOC(c, c->dH2all, sizeof(float) * M * H2);
        DALLOC(c, c->dXemb, sizeof(float) * M * c->ldX1);
        const int Hm = H1 > H2 ? H1 : H2;
        DALLOC(c, c->dhrec, sizeof(float) * B * Hm); DALLOC(c, c->dc, sizeof(float) * B * Hm);
        DALLOC(c, c->dxcnn, sizeof(float) * B * c->ldh); DALLOC(c, c->dxcT, es * h * c->ldB);
        int64_t ra = 4 * Hm; if (V > ra) ra = V;
        int64_t rb = 2 * H2; if (X1 + H1 > rb) rb = X1 + H1;  // stacked [x | h_prev]^T of one LSTM
        DALLOC(c, c->TA, es * ra * c->ldM);        DALLOC(c, c->TB, es * rb * c->ldM);
        DALLOC(c, c->logp, sizeof(double) * 2);
        DALLOC(c, c->zero_page, 256);
        if (hipMemset(c->zero_page, 0, 256) != hipSuccess) return LRCN_EHIP;
        for (auto &e : c->grad_ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return LRCN_EHIP;
        c->gemm_ws_bytes = 48u << 20;
        DALLOC(c, c->gemm_ws, c->gemm_ws_bytes);
        DALLOC(c, c->wg_ws, c->gemm_ws_bytes);
        if (hipStreamCreateWithFlags(&c->wg_stream, hipStreamNonBlocking) != hipSuccess) return LRCN_EHIP;
        for (auto &e : c->wg_fork)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return LRCN_EHIP;
        if (hipEventCreateWithFlags(&c->wg_done, hipEventDisableTiming) != hipSuccess) return LRCN_EHIP;
        if (hipEventCreateWithFlags(&c->xc_fork, hipEventDisableTiming) != hipSuccess) return LRCN_EHIP;
        if (hipEventCreateWithFlags(&c->xc_done, hipEventDisableTiming) != hipSuccess) return LRCN_EHIP;
        if (cfg->max_images > 0) DALLOC(c, c->vgg_ws, c->gemm_ws_bytes);
        for (int i = 0; i < 4; ++i) {
            DALLOC(c, c->st_f32[i], sizeof(float) * B * Hm);
            DALLOC(c, c->st2_f32[i], sizeof(float) * B * Hm);
        }
        DALLOC(c, c->st_h1, es * B * c->ldH1);     DALLOC(c, c->st_h2, es * B * c->ldH2);
        DALLOC(c, c->st_x, es * B * c->ldX1);      DALLOC(c, c->st_x2, es * B * c->ldH2);
        DALLOC(c, c->st_a, es * B * (c->ld4H1 > c->ld4H2 ? c->ld4H1 : c->ld4H2));
        DALLOC(c, c->st_g, sizeof(float) * B * 4 * Hm);
        DALLOC(c, c->st_logits, sizeof(float) * B * c->ldV); DALLOC(c, c->st_prob, sizeof(float) * B * c->ldV);
        int64_t io = (int64_t)B * (V > 4 * Hm ? V : 4 * Hm); if (io < (int64_t)B * (X1 + Hm)) io = (int64_t)B * (X1 + Hm);
        DALLOC(c, c->st_io, sizeof(float) * io);
        DALLOC(c, c->st_topi, sizeof(int32_t) * B * 32); DALLOC(c, c->st_topv, sizeof(float) * B * 32);
        DALLOC(c, c->st_parent, sizeof(int32_t) * B);
        for (int i = 0; i < 2; ++i) DALLOC(c, c->bs_seq[i], sizeof(int32_t) * B * LRCN_BEAM_MAXLEN);
        DALLOC(c, c->bs_last, sizeof(int32_t) * B);      DALLOC(c, c->bs_done, sizeof(int32_t) * B);
        DALLOC(c, c->bs_ndone, sizeof(int32_t) * 4);     DALLOC(c, c->bs_res_tok, sizeof(int32_t) * B * LRCN_BEAM_MAXLEN);
        DALLOC(c, c->bs_res_len, sizeof(int32_t) * B);   DALLOC(c, c->bs_p, sizeof(float) * B);
        DALLOC(c, c->bs_res_p, sizeof(float) * B);
        if (cfg->max_images > 0) {
            const int64_t N = cfg->max_images;
            const size_t ve = c->vesz;
            if (c->vdt != GEMM_T_BF16) DALLOC(c, c->im2col, ve * N * 224 * 224 * 32);  // bf16 fuses conv1_1's im2col
            DALLOC(c, c->actA, ve * N * 224 * 224 * 64);
            if (c->vdt == GEMM_T_BF16) DALLOC(c, c->img16, 2 * (N * 228 * 228 * 3 + 8));  // mean-subtracted crops in a 2-pixel zero frame (fused conv1_1+conv1_2)
            DALLOC(c, c->actB, ve * N * 112 * 112 * 128);  // largest tensor ever written to the second buffer (pool1 out = N*112*112*64; conv2_1 out = N*112*112*128)
            DALLOC(c, c->f6, ve * N * 4096);
            DALLOC(c, c->featsRM, sizeof(float) * N * 4096);
            if (c->vgg_fp8) DALLOC(c, c->amax_dev, sizeof(float) * 16);
        }
        return LRCN_OK;
    }();
    if (rc) {
        g_create_err = c->err;
        lrcn_destroy(c);
        return rc;
    }
    *out = c;
    return LRCN_OK;
}

int lrcn_vgg_set_wg_cap(lrcn_ctx *c, int cap) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (cap < 0 || (cap > 0 && cap < 8)) FAIL(c, LRCN_EINVAL, "wg_cap=%d must be 0 (off) or >= 8", cap);
    c->vgg_wg_cap = cap;
    return LRCN_OK;
}

int lrcn_set_stream(lrcn_ctx *c, void *s) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    c->stream = reinterpret_cast<hipStream_t>(s);
    return LRCN_OK;
}
int lrcn_set_wg_stream(lrcn_ctx *c, void *s) {
    DeviceGuard dg(c);
    if (!c || !s) return LRCN_EINVAL;
    if (c->wg_stream) {
        HIPCHK(c, hipStreamSynchronize(c->wg_stream));
        if (c->wg_stream_owned) (void)hipStreamDestroy(c->wg_stream);
    }
    c->wg_stream = reinterpret_cast<hipStream_t>(s);
    c->wg_stream_owned = false;
    return LRCN_OK;
}
int lrcn_sync(lrcn_ctx *c) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    return fetch_loss(c, nullptr);  // synchronises, and reports a pending out-of-range-token error
}

int lrcn_init_weights(lrcn_ctx *c, float *const p[9], uint64_t seed) {
    DeviceGuard dg(c);
    if (!c || !p) return LRCN_EINVAL;
    int64_t sz[9];
    ctx_sizes(c, sz);
    const int E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V;
    const int rows[9] = {c->X1 + H1, 1, 2 * H2, 1, H1, LRCN_CNNOUT, V, H2, 1};
    const int cols[9] = {4 * H1, 4 * H1, 4 * H2, 4 * H2, h, h, E, V, V};
    for (int k = 0; k < 9; ++k) {
        if (sz[k] == 0) continue;  // LRCN-1f has no W2 / b2 / Wproj
        if (!p[k]) FAIL(c, LRCN_EINVAL, "null parameter tensor %d", k);
        if (k == 1 || k == 3 || k == 8) {
            k_fill(c->stream, p[k], sz[k], 0.0f);
            if (k != 8) k_fill(c->stream, p[k], k == 1 ? H1 : H2, 1.0f);  // forget-gate bias = 1 (lrcn.jl:501)
        } else {
            k_init_uniform(c->stream, p[k], sz[k], (float)std::sqrt(2.0 / ((double)rows[k] + (double)cols[k])), seed, k);
        }
    }
    KCHK(c, "init_weights");
    c->shadow_valid = false;
    c->fused_groups = 0;
    return LRCN_OK;
}

int lrcn_loss(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, int norm_B,
              const lrcn_dropout *drop, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || (!tokens && T > 0)) return LRCN_EINVAL;
    int r = loss_impl(c, p, feats, tokens, T, B, norm_B, drop, nullptr, nullptr);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_loss_grad(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, int norm_B,
                   const lrcn_dropout *drop, float *const grads[9], double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || (!tokens && T > 0) || !grads) return LRCN_EINVAL;
    int r = loss_impl(c, p, feats, tokens, T, B, norm_B, drop, grads, nullptr);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

// ---- include/lrcn_varlen.h: per-row caption lengths ----
int lrcn_loss_var(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B,
                  int64_t norm_tokens, const lrcn_dropout *drop, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || (!tokens && T > 0)) return LRCN_EINVAL;
    if (!lens) FAIL(c, LRCN_EINVAL, "lens is NULL");
    int r = loss_impl(c, p, feats, tokens, T, B, 1, drop, nullptr, nullptr, lens, norm_tokens);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_loss_grad_var(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B,
                       int64_t norm_tokens, const lrcn_dropout *drop, float *const grads[9], double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || (!tokens && T > 0) || !grads) return LRCN_EINVAL;
    if (!lens) FAIL(c, LRCN_EINVAL, "lens is NULL");
    int r = loss_impl(c, p, feats, tokens, T, B, 1, drop, grads, nullptr, lens, norm_tokens);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_grad_group_wait(lrcn_ctx *c, int group, void *stream) {
    DeviceGuard dg(c);
    if (!c || group < 0 || group >= LRCN_GRAD_GROUPS) return LRCN_EINVAL;
    HIPCHK(c, hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), c->grad_ev[group], 0));
    return LRCN_OK;
}

int lrcn_last_loss(lrcn_ctx *c, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !loss_host) return LRCN_EINVAL;
    return fetch_loss(c, loss_host);
}

int lrcn_forward_logits(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B,
                        float *logits_out) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || (!tokens && T > 0) || !logits_out) return LRCN_EINVAL;
    return loss_impl(c, p, feats, tokens, T, B, B, nullptr, nullptr, logits_out);
}

// ---- include/lrcn_clip.h: the control block ----
namespace {
int ensure_clip(lrcn_ctx *c) {
    if (c->clip_ctl) return LRCN_OK;
    double *parts = nullptr;
    ClipCtl *ctl = nullptr;
    DALLOC(c, parts, sizeof(double) * LRCN_CLIP_SLOTS * kSumsqParts);
    DALLOC(c, ctl, sizeof(ClipCtl));
    ClipCtl init{};
    init.scale = 1.0f;  // an update that reads the block before any lrcn_clip_set is the plain update
    HIPCHK(c, hipMemcpy(ctl, &init, sizeof(init), hipMemcpyHostToDevice));
    c->clip_parts = parts;
    c->clip_ctl = ctl;
    return LRCN_OK;
}
inline hipStream_t stream_or_ctx(lrcn_ctx *c, void *stream) { return stream ? reinterpret_cast<hipStream_t>(stream) : c->stream; }

// the bodies of lrcn_adam_update / _group / _flat and of their clipped namesakes (clip: NULL or the context's control block)
int adam_update_impl(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step, float lr,
                     float b1, float b2, float eps, const ClipCtl *clip);
int adam_update_group_impl(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                           int step, float lr, float b1, float b2, float eps, void *stream, const ClipCtl *clip);
int adam_update_flat_impl(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1, float b2,
                          float eps, void *stream, const ClipCtl *clip);
}  // namespace

int lrcn_adam_update(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step,
                     float lr, float b1, float b2, float eps) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || step < 1) return LRCN_EINVAL;
    return adam_update_impl(c, p, g, m, v, step, lr, b1, b2, eps, nullptr);
}
namespace {
int adam_update_impl(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step, float lr,
                     float b1, float b2, float eps, const ClipCtl *clip) {
    c->fused_groups = 0;  // the whole-model update supersedes any per-group sequence left unfinished (an error between two groups)
    int64_t nparam = 0;
    {
        int64_t szp[9];
        ctx_sizes(c, szp);
        for (int k = 0; k < 9; ++k) nparam += szp[k];
    }
    SegScope seg(c, LRCN_SEG_UPDATE, c->stream, 28.0 * (double)nparam);  // w, m, v read + written, g read: 28 B per parameter
    if (c->opt_fused) {  // LRCN_OPT_FUSED_UPDATE: the same update, and the next step's shadow weights in the same pass
        c->shadow_valid = false;
        int r = adam_fused(c, p, g, m, v, -1, step, lr, b1, b2, eps, c->stream, clip);
        if (r) return r;
        fused_update_done(c, p);
        return LRCN_OK;
    }
    c->shadow_valid = false;
    AdamTensors t;
    int64_t sz[9];
    ctx_sizes(c, sz);
    for (int k = 0; k < 9; ++k) {
        t.w[k] = p[k];
        t.g[k] = g[k];
        t.m[k] = m[k];
        t.v[k] = v[k];
        t.n[k] = sz[k];
    }
    k_adam(c->stream, t, step, lr, b1, b2, eps, clip);
    KCHK(c, "adam");
    return LRCN_OK;
}
}  // namespace

int lrcn_adam_update_group(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                           int step, float lr, float b1, float b2, float eps, void *stream) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || step < 1) return LRCN_EINVAL;
    if (group < 0 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [0,%d)", group, LRCN_GRAD_GROUPS);
    return adam_update_group_impl(c, p, g, m, v, group, step, lr, b1, b2, eps, stream, nullptr);
}
namespace {
int adam_update_group_impl(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                           int step, float lr, float b1, float b2, float eps, void *stream, const ClipCtl *clip) {
    int64_t szg[9];
    ctx_sizes(c, szg);
    SegScope seg(c, LRCN_SEG_UPDATE, stream ? reinterpret_cast<hipStream_t>(stream) : c->stream,
                 28.0 * (double)(szg[kGradGroup[group][0]] + (kGradGroup[group][1] != kGradGroup[group][0] ? szg[kGradGroup[group][1]] : 0)));
    if (c->opt_fused) {
        // fused with the shadow pass; the written set becomes current once all five groups of this step have been issued (they are
        // issued in any order, each exactly once per step, with the same `step`)
        if (step != c->fused_step) {  // first group of a new step: bits left by a step that never completed do not count
            c->fused_groups = 0;
            c->fused_step = step;
        }
        c->shadow_valid = false;
        int r = adam_fused(c, p, g, m, v, group, step, lr, b1, b2, eps, stream ? reinterpret_cast<hipStream_t>(stream) : c->stream, clip);
        if (r) {
            c->fused_groups = 0;
            return r;
        }
        c->fused_groups |= 1u << group;
        if (c->fused_groups == (1u << LRCN_GRAD_GROUPS) - 1) {
            c->fused_groups = 0;
            fused_update_done(c, p);
        }
        return LRCN_OK;
    }
    c->shadow_valid = false;
    AdamTensors t;
    int64_t sz[9];
    ctx_sizes(c, sz);
    for (int k = 0; k < 9; ++k) {
        const bool in = k == kGradGroup[group][0] || k == kGradGroup[group][1];
        t.w[k] = p[k];
        t.g[k] = g[k];
        t.m[k] = m[k];
        t.v[k] = v[k];
        t.n[k] = in ? sz[k] : 0;
    }
    k_adam(stream ? reinterpret_cast<hipStream_t>(stream) : c->stream, t, step, lr, b1, b2, eps, clip);
    KCHK(c, "adam (group)");
    return LRCN_OK;
}
}  // namespace

int lrcn_refresh_shadows_group(lrcn_ctx *c, const float *const p[9], int group, void *stream) {
    DeviceGuard dg(c);
    if (!c || !p) return LRCN_EINVAL;
    if (group < 0 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [0,%d)", group, LRCN_GRAD_GROUPS);
    if (!c->opt_fused) FAIL(c, LRCN_ESTATE, "lrcn_refresh_shadows_group needs LRCN_OPT_FUSED_UPDATE = 1 (the second shadow set)");
    int r = ensure_alt_shadows(c);
    if (r) return r;
    if (c->refresh_groups == 0) c->shadow_valid = false;  // first group of a step: the current set describes the OLD parameters from now on
    PrepPlan plan{};
    if (c->gi_live && (r = ensure_gi_sets(c))) return r;
    plan_matrices(c, p, alt_shadows(c), true, plan, kGradGroup[group][0], kGradGroup[group][1], c->gi_live ? c->alt_gi : nullptr);
    if (plan.n > 0) {  // LRCN-1f has no W2 / Wproj: an empty group is only counted
        k_prepare_weights(stream ? reinterpret_cast<hipStream_t>(stream) : c->stream, c->dt, plan);
        KCHK(c, "refresh_shadows_group");
    }
    c->refresh_groups |= 1u << group;
    if (c->refresh_groups == (1u << LRCN_GRAD_GROUPS) - 1) {
        c->refresh_groups = 0;
        float *pp[9];
        for (int k = 0; k < 9; ++k) pp[k] = const_cast<float *>(p[k]);
        fused_update_done(c, pp);
    }
    return LRCN_OK;
}

int lrcn_adam_update_flat(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1, float b2,
                          float eps, void *stream) {
    DeviceGuard dg(c);
    if (!c || step < 1 || n < 0) return LRCN_EINVAL;
    if (n == 0) return LRCN_OK;
    if (!w || !g || !m || !v) return LRCN_EINVAL;
    return adam_update_flat_impl(c, w, g, m, v, n, step, lr, b1, b2, eps, stream, nullptr);
}
namespace {
int adam_update_flat_impl(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1, float b2,
                          float eps, void *stream, const ClipCtl *clip) {
    c->shadow_valid = false;  // some parameter changed: the next call makes its shadow weights afresh
    SegScope seg(c, LRCN_SEG_UPDATE, stream ? reinterpret_cast<hipStream_t>(stream) : c->stream, 28.0 * (double)n);
    AdamTensors t{};
    t.w[0] = w; t.g[0] = g; t.m[0] = m; t.v[0] = v; t.n[0] = n;
    k_adam(stream ? reinterpret_cast<hipStream_t>(stream) : c->stream, t, step, lr, b1, b2, eps, clip);
    KCHK(c, "adam (flat)");
    return LRCN_OK;
}
}  // namespace

int lrcn_train_step(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                    const int32_t *tokens, int T, int B, int norm_B, const lrcn_dropout *drop, int step, float lr, float b1,
                    float b2, float eps, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v) return LRCN_EINVAL;
    int r = lrcn_loss_grad(c, p, feats, tokens, T, B, norm_B, drop, g, nullptr);
    if (r) return r;
    r = lrcn_adam_update(c, p, g, m, v, step, lr, b1, b2, eps);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_train_step_var(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                        const int32_t *tokens, const int32_t *lens, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, int step,
                        float lr, float b1, float b2, float eps, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v) return LRCN_EINVAL;
    int r = lrcn_loss_grad_var(c, p, feats, tokens, lens, T, B, norm_tokens, drop, g, nullptr);
    if (r) return r;
    r = lrcn_adam_update(c, p, g, m, v, step, lr, b1, b2, eps);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

// ---- include/lrcn_clip.h: global gradient-norm clipping ----
int lrcn_grad_sumsq(lrcn_ctx *c, const float *g, int64_t n, int slot, void *stream) {
    DeviceGuard dg(c);
    if (!c || n < 0 || (!g && n > 0)) return LRCN_EINVAL;
    if (slot < 0 || slot >= LRCN_CLIP_SLOTS) FAIL(c, LRCN_EINVAL, "slot=%d outside [0,%d)", slot, LRCN_CLIP_SLOTS);
    int r = ensure_clip(c);
    if (r) return r;
    SumsqArgs a{};
    a.g[0] = g; a.n[0] = n; a.slot[0] = slot; a.count = 1;
    k_sumsq(stream_or_ctx(c, stream), a, c->clip_parts, c->clip_ctl);
    KCHK(c, "sumsq");
    return LRCN_OK;
}

int lrcn_grad_sumsq_model(lrcn_ctx *c, const float *const g[9], int group, void *stream) {
    DeviceGuard dg(c);
    if (!c || !g) return LRCN_EINVAL;
    if (group < -1 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [-1,%d)", group, LRCN_GRAD_GROUPS);
    int64_t sz[9];
    ctx_sizes(c, sz);
    SumsqArgs a{};
    for (int k = 0; k < 9; ++k) {
        if (group >= 0 && k != kGradGroup[group][0] && k != kGradGroup[group][1]) continue;
        if (sz[k] > 0 && !g[k]) return LRCN_EINVAL;
        a.g[a.count] = g[k]; a.n[a.count] = sz[k]; a.slot[a.count] = k;
        ++a.count;
    }
    int r = ensure_clip(c);
    if (r) return r;
    k_sumsq(stream_or_ctx(c, stream), a, c->clip_parts, c->clip_ctl);
    KCHK(c, "sumsq (model)");
    return LRCN_OK;
}

int lrcn_clip_slots(lrcn_ctx *c, double **dev_ptr) {
    DeviceGuard dg(c);
    if (!c || !dev_ptr) return LRCN_EINVAL;
    int r = ensure_clip(c);
    if (r) return r;
    *dev_ptr = c->clip_ctl->slot;  // (address arithmetic only: the block is never read from the host here)
    return LRCN_OK;
}

int lrcn_clip_set(lrcn_ctx *c, int n_slots, float max_norm, void *stream) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (n_slots < 1 || n_slots > LRCN_CLIP_SLOTS) FAIL(c, LRCN_EINVAL, "n_slots=%d outside [1,%d]", n_slots, LRCN_CLIP_SLOTS);
    if (!(max_norm > 0.0f)) FAIL(c, LRCN_EINVAL, "max_norm=%g is not > 0", (double)max_norm);
    int r = ensure_clip(c);
    if (r) return r;
    k_clip_set(stream_or_ctx(c, stream), c->clip_ctl, n_slots, max_norm);
    KCHK(c, "clip_set");
    return LRCN_OK;
}

int lrcn_adam_update_clipped(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step,
                             float lr, float b1, float b2, float eps) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || step < 1) return LRCN_EINVAL;
    int r = ensure_clip(c);
    if (r) return r;
    return adam_update_impl(c, p, g, m, v, step, lr, b1, b2, eps, c->clip_ctl);
}

int lrcn_adam_update_group_clipped(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                                   int step, float lr, float b1, float b2, float eps, void *stream) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || step < 1) return LRCN_EINVAL;
    if (group < 0 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [0,%d)", group, LRCN_GRAD_GROUPS);
    int r = ensure_clip(c);
    if (r) return r;
    return adam_update_group_impl(c, p, g, m, v, group, step, lr, b1, b2, eps, stream, c->clip_ctl);
}

int lrcn_adam_update_flat_clipped(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1,
                                  float b2, float eps, void *stream) {
    DeviceGuard dg(c);
    if (!c || step < 1 || n < 0) return LRCN_EINVAL;
    if (n == 0) return LRCN_OK;
    if (!w || !g || !m || !v) return LRCN_EINVAL;
    int r = ensure_clip(c);
    if (r) return r;
    return adam_update_flat_impl(c, w, g, m, v, n, step, lr, b1, b2, eps, stream, c->clip_ctl);
}

namespace {
// the nine sums of squares, norm / scale / skip and the clipped update of one training step, all on the context's stream
int clip_and_update(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], int step, float lr, float b1,
                    float b2, float eps, float max_norm) {
    int r = lrcn_grad_sumsq_model(c, g, -1, nullptr);
    if (r || (r = lrcn_clip_set(c, LRCN_CLIP_SLOTS, max_norm, nullptr))) return r;
    return lrcn_adam_update_clipped(c, p, g, m, v, step, lr, b1, b2, eps);
}
}  // namespace

int lrcn_train_step_clip(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                         const int32_t *tokens, int T, int B, int norm_B, const lrcn_dropout *drop, int step, float lr, float b1, float b2,
                         float eps, float max_norm, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v) return LRCN_EINVAL;
    if (std::isnan(max_norm)) FAIL(c, LRCN_EINVAL, "max_norm is NaN");
    if (!(max_norm > 0.0f)) return lrcn_train_step(c, p, g, m, v, feats, tokens, T, B, norm_B, drop, step, lr, b1, b2, eps, loss_host);
    if (step < 1) return LRCN_EINVAL;
    int r = lrcn_loss_grad(c, p, feats, tokens, T, B, norm_B, drop, g, nullptr);
    if (r || (r = clip_and_update(c, p, g, m, v, step, lr, b1, b2, eps, max_norm))) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_train_step_var_clip(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                             const int32_t *tokens, const int32_t *lens, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop,
                             int step, float lr, float b1, float b2, float eps, float max_norm, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v) return LRCN_EINVAL;
    if (std::isnan(max_norm)) FAIL(c, LRCN_EINVAL, "max_norm is NaN");
    if (!(max_norm > 0.0f))
        return lrcn_train_step_var(c, p, g, m, v, feats, tokens, lens, T, B, norm_tokens, drop, step, lr, b1, b2, eps, loss_host);
    if (step < 1) return LRCN_EINVAL;
    int r = lrcn_loss_grad_var(c, p, feats, tokens, lens, T, B, norm_tokens, drop, g, nullptr);
    if (r || (r = clip_and_update(c, p, g, m, v, step, lr, b1, b2, eps, max_norm))) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_clip_stats(lrcn_ctx *c, lrcn_clip_stats_t *out) {
    DeviceGuard dg(c);
    if (!c || !out) return LRCN_EINVAL;
    int r = ensure_clip(c);
    if (r) return r;
    ClipCtl h{};
    HIPCHK(c, hipMemcpyAsync(&h, c->clip_ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->last_norm = h.norm;
    out->last_scale = h.scale;
    out->last_skipped = h.skip;
    out->steps = h.steps;
    out->clipped = h.clipped;
    out->skipped = h.skipped;
    return LRCN_OK;
}

int lrcn_comm_unique_id(void *id_out) {
    if (!id_out) return LRCN_EINVAL;
    char err[256] = "";
    if (comm_unique_id(id_out, err, sizeof(err))) {
        g_create_err = err;
        return LRCN_EHIP;
    }
    return LRCN_OK;
}

int lrcn_comm_probe(lrcn_ctx *c) {
    if (!c) return LRCN_EINVAL;
    if (c->comm) FAIL(c, LRCN_ESTATE, "the context already has a communicator");
    char err[256] = "";
    if (comm_available(err, sizeof(err))) FAIL(c, LRCN_EHIP, "%s", err);
    return LRCN_OK;
}

int lrcn_comm_init(lrcn_ctx *c, int world, int rank, const void *unique_id) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (world < 1 || rank < 0 || rank >= world || !unique_id) FAIL(c, LRCN_EINVAL, "comm_init: world=%d rank=%d", world, rank);
    if (c->comm) FAIL(c, LRCN_ESTATE, "the context already has a communicator");
    char err[256] = "";
    c->comm = comm_create(world, rank, unique_id, err, sizeof(err));
    if (!c->comm) FAIL(c, LRCN_EHIP, "%s", err);
    return ensure_buckets(c);
}

int lrcn_set_embed_rows_buffer(lrcn_ctx *c, float *rows, int32_t *tok, int capacity_rows) {
    if (!c) return LRCN_EINVAL;
    if ((rows == nullptr) != (tok == nullptr) || capacity_rows < 0) FAIL(c, LRCN_EINVAL, "rows and tok must both be given (capacity >= 0) or both NULL");
    c->emb_rows_out = rows;
    c->emb_tok_out = tok;
    c->emb_rows_cap = rows ? capacity_rows : 0;
    return LRCN_OK;
}

int lrcn_embed_grad_from_rows(lrcn_ctx *c, const float *rows, const int32_t *tok, int n_rows, float *grad_wembed, void *stream) {
    DeviceGuard dg(c);
    if (!c || !rows || !tok || !grad_wembed) return LRCN_EINVAL;
    if (n_rows < 1 || n_rows > 8192) FAIL(c, LRCN_EINVAL, "n_rows=%d outside [1, 8192] (the ordered sum ranks at most 8192 keys)", n_rows);
    if (!c->dWe_rm) DALLOC(c, c->dWe_rm, sizeof(float) * (size_t)c->V * c->ldE);
    if (!c->imp_keys) DALLOC(c, c->imp_keys, sizeof(unsigned long long) * 8192);
    hipStream_t st = stream ? reinterpret_cast<hipStream_t>(stream) : c->stream;
    DropSpec none{};
    // ordered: every rank sums the same rows in the same order -> bit-identical dense gradients (what an all-reduce guarantees)
    if (!k_embed_scatter_rm(st, rows, c->E, tok, n_rows, 1, c->E, c->V, none, c->dWe_rm, c->ldE, grad_wembed, c->imp_keys))
        FAIL(c, LRCN_EINVAL, "embed_grad_from_rows: too many rows (%d)", n_rows);
    KCHK(c, "embed_grad_from_rows");
    return LRCN_OK;
}

int lrcn_comm_set_stream(lrcn_ctx *c, void *hip_stream) {
    DeviceGuard dg(c);
    if (!c || !hip_stream) return LRCN_EINVAL;
    for (bool p : c->bucket_pending)
        if (p) FAIL(c, LRCN_ESTATE, "a gradient exchange is in flight: call lrcn_comm_join first");
    if (c->comm_stream && c->comm_stream_owned) {
        HIPCHK(c, hipStreamSynchronize(c->comm_stream));
        (void)hipStreamDestroy(c->comm_stream);
    }
    c->comm_stream = reinterpret_cast<hipStream_t>(hip_stream);
    c->comm_stream_owned = false;
    return ensure_buckets(c);
}

int lrcn_comm_destroy(lrcn_ctx *c) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());
    comm_destroy(c->comm);
    c->comm = nullptr;
    return LRCN_OK;
}

int lrcn_allreduce_grads(lrcn_ctx *c, float *const grads[9], int group) {
    DeviceGuard dg(c);
    if (!c || !grads) return LRCN_EINVAL;
    if (group < -1 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [-1,%d)", group, LRCN_GRAD_GROUPS);
    int r = ensure_buckets(c);
    if (r) return r;
    for (int g = (group < 0 ? 0 : group); g < (group < 0 ? LRCN_GRAD_GROUPS : group + 1); ++g) {
        r = allreduce_group(c, grads, g);
        if (r) return r;
    }
    return LRCN_OK;
}

int lrcn_comm_join(lrcn_ctx *c) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    return join_buckets(c);
}

int lrcn_lstm(lrcn_ctx *c, const float *W, const float *b, int X, int H, int B, const float *x, const float *h, const float *cc,
              float *h_out, float *c_out) {
    DeviceGuard dg(c);
    if (!c || !W || !b || !x || !h || !cc || !h_out || !c_out) return LRCN_EINVAL;
    void *Wx, *Wh, *xb, *hb;
    if (X == c->X1 && H == c->H1) {
        Wx = c->W1x; Wh = c->W1h; xb = c->st_x; hb = c->st_h1;
    } else if (c->nl == 2 && X == c->H2 && H == c->H2) {
        Wx = c->W2x; Wh = c->W2h; xb = c->st_x2; hb = c->st_h2;
    } else {
        FAIL(c, LRCN_EINVAL, "lrcn_lstm: (X=%d,H=%d) must be the context's LSTM-1 (%d,%d) or (two layers) LSTM-2 (%d,%d)", X, H, c->X1, c->H1,
             c->H2, c->H2);
    }
    if (B < 1 || B > c->maxB) FAIL(c, LRCN_EINVAL, "B=%d outside [1,%d]", B, c->maxB);
    const int dt = c->dt;
    hipStream_t st = c->stream;
    const int64_t ldX = ld64(X), ldH = ld64(H);
    // shadows of this W: memory [4H][X+H]
    c->shadow_valid = false;
    k_cast_rows(st, dt, W, X + H, 4 * H, X, Wx, ldX);
    k_cast_rows(st, dt, W + X, X + H, 4 * H, H, Wh, ldH);
    // x (B x X column-major = memory [X][B]) -> [B][ldX] T ; h likewise ; c -> f32 row-major
    k_transpose(st, dt, 1, x, B, X, B, xb, ldX, 0);
    k_transpose(st, dt, 1, h, B, H, B, hb, ldH, 0);
    k_transpose_f32(st, cc, B, H, B, c->st_f32[1], H);
    GEMM(c, dt, xb, ldX, Wx, ldX, c->st_g, 4 * H, B, 4 * H, X, b, true);
    GEMM(c, dt, hb, ldH, Wh, ldH, c->st_g, 4 * H, B, 4 * H, H, nullptr, true, true);
    k_lstm_fwd(st, dt, c->st_g, 4 * H, c->st_f32[1], B, H, c->st_a, ld64(4 * H), c->st_f32[1], hb, ldH, c->st_f32[0]);
    k_transpose_f32(st, c->st_f32[0], H, B, H, h_out, B);
    k_transpose_f32(st, c->st_f32[1], H, B, H, c_out, B);
    KCHK(c, "lrcn_lstm");
    return LRCN_OK;
}

int lrcn_step(lrcn_ctx *c, const float *const p[9], float *const state[4], int B, const float *x_cnn, const float *x_lstm,
              const float *mask1, const float *mask2, float *logits) {
    DeviceGuard dg(c);
    if (!c || !p || !state || !x_cnn || !x_lstm || !logits) return LRCN_EINVAL;
    if (B < 1 || B > c->maxB) FAIL(c, LRCN_EINVAL, "B=%d outside [1,%d]", B, c->maxB);
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V;
    hipStream_t st = c->stream;
    int r = prepare_weights(c, p, false);
    if (r) return r;
    const int Hs[4] = {H1, H1, H2, H2};
    const int ns = c->nl == 1 ? 2 : 4;  // LRCN-1f: state = {h, c}
    for (int i = 0; i < ns; ++i) {
        if (!state[i]) FAIL(c, LRCN_EINVAL, "null state tensor %d", i);
        k_transpose_f32(st, state[i], B, Hs[i], B, c->st_f32[i], Hs[i]);
    }
    k_transpose_f32(st, x_cnn, B, h, B, c->xcnn, c->ldh);
    // two layers: x = dropout(x_lstm)  (lrcn.jl:542): both arrays are B x E column-major, multiply first, then lay out [B][ldE] (T);
    // mask2 (B x H2) multiplies the concatenated LSTM-2 input (:547).  LRCN-1f: mask1 (B x (E+h)) multiplies hcat(x_lstm, x_cnn).
    DropSpec d2{};
    d2.which = c->nl == 1 ? 1 : 2;
    d2.mask = c->nl == 1 ? mask1 : mask2;
    const float *xsrc = x_lstm;
    if (mask1 && c->nl == 2) {
        k_mul_f32(st, x_lstm, mask1, (int64_t)B * E, c->st_io);
        xsrc = c->st_io;
    }
    k_transpose(st, dt, 1, xsrc, B, E, B, c->st_x, c->ldX1, 0);
    r = step_internal(c, p, B, d2);
    if (r) return r;
    for (int i = 0; i < ns; ++i) k_transpose_f32(st, c->st_f32[i], Hs[i], B, Hs[i], state[i], B);
    k_transpose_f32(st, c->st_logits, c->ldV, B, V, logits, B);
    KCHK(c, "lrcn_step");
    return LRCN_OK;
}

int lrcn_train_step_dp(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const uint8_t *img_u8,
                       const float mean[3], int normalize, float *feats, const int32_t *tokens, int T, int B, int norm_B,
                       const lrcn_dropout *drop, int step, float lr, float b1, float b2, float eps, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || !feats || step < 1) return LRCN_EINVAL;
    int r;
    if (img_u8) {  // [VGG forward of this rank's crops] -> feats
        if (!mean && !c->avg_on) FAIL(c, LRCN_EINVAL, "img_u8 given without channel means or an averageImage");
        r = vgg_check(c, B);
        if (r) return r;
        r = vgg_body(c, B, img_u8, true, mean);
        if (r) return r;
        k_transpose_f32(c->stream, c->featsRM, 4096, B, 4096, feats, B);
        if (normalize) k_normalize_rows(c->stream, feats, B, LRCN_CNNOUT);
        KCHK(c, "train_step_dp (vgg)");
    }
    r = loss_impl(c, p, feats, tokens, T, B, norm_B, drop, g, nullptr);
    if (r) return r;
    if (!c->comm || (comm_world(c->comm) == 1 && !dp_force_pipeline())) {  // one rank: nothing to hide the update behind -- one Adam launch
        r = lrcn_adam_update(c, p, g, m, v, step, lr, b1, b2, eps);
        if (r) return r;
        return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
    }
    // per gradient group, on its own stream, while the rest of the backward pass is still running on the context's stream:
    // [wait for the group's gradients] -> [all-reduce over xGMI] -> [Adam of that group].  The backward reads the shadows made
    // at the start of the step, never the f32 parameters, so updating a group early is safe.
    r = ensure_buckets(c);
    if (r) return r;
    for (int grp = 0; grp < LRCN_GRAD_GROUPS; ++grp) {
        r = allreduce_group(c, g, grp);
        if (r) return r;
        r = lrcn_adam_update_group(c, p, g, m, v, grp, step, lr, b1, b2, eps, c->bucket[grp]);
        if (r) return r;
    }
    r = join_buckets(c);  // the next step's shadow-weight pass reads the updated parameters
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

int lrcn_debug_stamps(lrcn_ctx *c, unsigned long long *host_out, int64_t n) {
    DeviceGuard dg(c);
    if (!c || !host_out || n < 1) return LRCN_EINVAL;
    if (!c->stamps || n > c->stamps_n) FAIL(c, LRCN_ESTATE, "no stamps recorded (LRCN_STAMPS=1 and lrcn_bench_conv first), or n > %lld", (long long)c->stamps_n);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(host_out, c->stamps, sizeof(unsigned long long) * (size_t)n, hipMemcpyDeviceToHost));
    return LRCN_OK;
}

const char *lrcn_debug_route(lrcn_ctx *c, int which) {
    if (which == 1) return c ? c->vgg_routes.c_str() : "";
    return gemm_debug_last_route();
}

int lrcn_profile(lrcn_ctx *c, int enable) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    c->prof = enable != 0;
    c->prof_level = enable;
    c->prof_used = 0;
    c->prof_ms = 0.0;
    c->prof_launches = 0;
    for (auto &sp : c->seg) {
        sp.used = 0;
        sp.ms = sp.bytes = 0.0;
        sp.n = 0;
    }
    return LRCN_OK;
}

int lrcn_profile_segment(lrcn_ctx *c, int segment, double *ms, int64_t *brackets, double *bytes) {
    DeviceGuard dg(c);
    if (!c || !ms || !brackets || !bytes || segment < 0 || segment >= LRCN_SEG_COUNT) return LRCN_EINVAL;
    HIPCHK(c, hipDeviceSynchronize());  // the segments live on several streams (context, copy, caller-given update streams)
    auto &sp = c->seg[segment];
    for (size_t i = 0; i < sp.used; ++i) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, sp.ev[i].first, sp.ev[i].second));
        sp.ms += t;
    }
    sp.used = 0;
    *ms = sp.ms;
    *brackets = sp.n;
    *bytes = sp.bytes;
    return LRCN_OK;
}

int lrcn_avg_loss_batch(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, double *loss_host) {
    // average_loss's loop body (lrcn.jl:452-475): pdrop 0, normalised by the batch's own size (lrcn.jl:412)
    return lrcn_loss(c, p, feats, tokens, T, B, B, nullptr, loss_host);
}

int lrcn_profile_get(lrcn_ctx *c, double *conv_ms, int64_t *conv_launches) {
    DeviceGuard dg(c);
    if (!c || !conv_ms || !conv_launches) return LRCN_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->prof_used; ++i) {
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->prof_ev[i].first, c->prof_ev[i].second));
        c->prof_ms += ms;
        c->prof_launches += 12;
    }
    c->prof_used = 0;
    *conv_ms = c->prof_ms;
    *conv_launches = c->prof_launches;
    return LRCN_OK;
}

}  // extern "C"
