// lrcn_api.hip -- the caption model's context behind the C ABI of liblrcn_hip.so (include/lrcn.h): its creation, options, streams and
// workspace, the GEMM helper every host file of the model launches its contractions through, the reference's single-step functions
// (lrcn_lstm, lrcn_step) and the debug / profile getters.  The training step is train.hip (forward / backward pass), update.hip (shadow
// weights, Adam, clipping) and train_dp.hip (data parallelism); decoding is decode.hip, the VGG-16 forward vgg.hip.
#include <algorithm>
#include <cmath>

#include "ctx.h"

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

void lrcn_impl::set_create_error(const char *msg) { g_create_err = msg; }

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
    if (c->xl_arena) (void)hipFree(c->xl_arena);
    if (c->cn_arena) (void)hipFree(c->cn_arena);
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
    if (c->roww_pin) (void)hipHostFree(c->roww_pin);
    for (auto &e : c->roww_up)
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
    int r = prepare_weights(c, p);   // the forward shadows alone
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
