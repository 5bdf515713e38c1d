// train.hip -- the caption model's forward / backward pass on one gfx950 device, and its loss and train-step entry points (include/lrcn.h,
// lrcn_varlen.h, lrcn_clip.h, lrcn_weighted.h, lrcn_sched.h, lrcn_smooth.h), each of which describes its call in one LossCall (ctx.h) filled by member name.
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
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "../../include/lrcn_varlen.h"
#include "../../include/lrcn_clip.h"
#include "../../include/lrcn_weighted.h"
#include "../../include/lrcn_sched.h"
#include "../../include/lrcn_smooth.h"

using namespace lrcn_impl;

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
// The same forward epilogue IS the default of the batched beam decode (decode.hip decode_gates_epi), where its GEMMs fill the chip.
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

// What the cell-epilogue and K-slab launches of one timestep share: M = B rows of A starting at row s*B, the recurrent weights W [N][ld],
// both K-contiguous with the same leading dimension.  Each route then sets only what is its own.
GemmArgs rec_step_args(lrcn_ctx *c, const void *A, int64_t ld, int s, int B, const void *W, int N, int K) {
    GemmArgs g{};
    g.dtype = c->dt;
    g.A = boff(A, (int64_t)s * B * ld, c->esz); g.lda = ld;
    g.B = W; g.ldb = ld;
    g.M = B; g.N = N; g.K = K;
    g.a_mode = GEMM_A_PLAIN;
    g.zero_page = c->zero_page;
    return g;
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
        GemmArgs g = rec_step_args(c, Hall, ldH, s - 1, B, Wh_gi, 4 * H, (int)ldH);
        g.out_mode = GEMM_OUT_LSTM_FWD;
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
            GemmArgs g = rec_step_args(c, dZ, ld4H, s, B, WhT, H, (int)ld4H);
            g.out_mode = GEMM_OUT_LSTM_BWD;
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
                    GemmArgs g = rec_step_args(c, dZ, ld4H, s, B, WhT, H, Kp);
                    g.C = slabs; g.ldc = H; g.c_f32 = 1;   // (unused: the slabs are the output)
                    g.out_mode = GEMM_OUT_PLAIN;
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

// B per-row values (host; int32 lengths or f32 weights) -> dev [maxB] on the context's stream, through the next pinned slot of their ring
template <typename E>
int upload_rows(lrcn_ctx *c, const E *host, int B, E *&dev, E *&pin, hipEvent_t (&up)[lrcn_ctx::kLenSlots], int &next) {
    // each piece on its own guard: a call that failed half-way through here leaves the next one to create what is still missing
    if (!dev) DALLOC(c, dev, sizeof(E) * (size_t)c->maxB);
    if (!pin) HIPCHK(c, hipHostMalloc((void **)&pin, sizeof(E) * (size_t)c->maxB * lrcn_ctx::kLenSlots, hipHostMallocDefault));
    for (auto &e : up)
        if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int k = next;
    next = (k + 1) % lrcn_ctx::kLenSlots;
    HIPCHK(c, hipEventSynchronize(up[k]));  // returns at once for an event never recorded
    E *slot = pin + (size_t)k * c->maxB;
    std::memcpy(slot, host, sizeof(E) * (size_t)B);
    HIPCHK(c, hipMemcpyAsync(dev, slot, sizeof(E) * (size_t)B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(up[k], c->stream));
    return LRCN_OK;
}
int upload_lens(lrcn_ctx *c, const int32_t *lens, int B) { return upload_rows(c, lens, B, c->lens_dev, c->lens_pin, c->lens_up, c->lens_slot); }
int upload_row_w(lrcn_ctx *c, const float *w, int B) { return upload_rows(c, w, B, c->roww_dev, c->roww_pin, c->roww_up, c->roww_slot); }

}  // namespace

// loss / lossgradient on internal buffers, described by a LossCall (ctx.h).  q.feats: B x 4096 column-major f32 (device).
// q.lens (host, [B]): the variable-length form of include/lrcn_varlen.h -- row b has lens[b] + 1 loss terms, the scale is
// 1 / norm_tokens and norm_B is not used.  Only the token builder and the softmax-NLL kernel differ; every launch in between is the same.
// q.row_w (host, [B], with lens): the weighted form of include/lrcn_weighted.h -- caption b's terms and d(logits) rows carry
// row_w[b]; the chain after the softmax-NLL kernel is linear in d(logits), so only that launch differs.
// q.ss (with lens): scheduled sampling of include/lrcn_sched.h.  eps == 0 changes nothing but the counters and fed_out; eps > 0 runs
// the forward step by step (sched_forward below) into the same buffers and rejoins at the softmax-NLL launch.
// q.smooth > 0 (with lens): label smoothing of include/lrcn_smooth.h -- again only the softmax-NLL launch differs.
int lrcn_impl::loss_impl(lrcn_ctx *c, const LossCall &q) {
    const int T = q.T, B = q.B;
    int r = check_shapes(c, T, B, q.norm_B);
    if (r) return r;
    if (q.ss) {
        if (!q.lens) FAIL(c, LRCN_EINVAL, "scheduled sampling needs lens");
        if (!(q.ss->eps >= 0.0f && q.ss->eps <= 1.0f)) FAIL(c, LRCN_EINVAL, "sched eps=%g outside [0,1]", (double)q.ss->eps);
        if (!(q.ss->temperature >= 0.0f) || std::isinf(q.ss->temperature))
            FAIL(c, LRCN_EINVAL, "sched temperature=%g must be finite and >= 0", (double)q.ss->temperature);
        if (q.ss->row0 < 0 || q.ss->row0 > ((int64_t)1 << 32) - B)
            FAIL(c, LRCN_EINVAL, "sched row0=%lld: rows [row0, row0 + B) must lie in [0, 2^32)", (long long)q.ss->row0);
    }
    const bool stepwise = q.ss && q.ss->eps > 0.0f;
    if (q.lens) {
        if (q.norm_tokens < 1) FAIL(c, LRCN_EINVAL, "norm_tokens=%lld must be >= 1", (long long)q.norm_tokens);
        for (int b = 0; b < B; ++b)
            if (q.lens[b] < 0 || q.lens[b] > T) FAIL(c, LRCN_EINVAL, "lens[%d]=%d outside [0,%d]", b, q.lens[b], T);
    }
    if (q.row_w) {
        if (!q.lens) FAIL(c, LRCN_EINVAL, "row weights need lens");
        for (int b = 0; b < B; ++b)
            if (!std::isfinite(q.row_w[b])) FAIL(c, LRCN_EINVAL, "row_w[%d]=%g is not finite", b, (double)q.row_w[b]);
    }
    if (!(q.smooth >= 0.0f && q.smooth <= 1.0f)) FAIL(c, LRCN_EINVAL, "smooth=%g outside [0,1]", (double)q.smooth);
    if (q.smooth > 0.0f && !q.lens) FAIL(c, LRCN_EINVAL, "label smoothing needs lens");
    if (q.drop && (q.drop->pdrop < 0.0f || q.drop->pdrop >= 1.0f)) FAIL(c, LRCN_EINVAL, "pdrop=%g outside [0,1)", q.drop->pdrop);
    if (q.drop && c->nl == 2 && ((q.drop->mask1 == nullptr) != (q.drop->mask2 == nullptr))) FAIL(c, LRCN_EINVAL, "mask1/mask2 must both be set");
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    const int S = T + 1, M = S * B;
    const size_t es = c->esz;
    hipStream_t st = c->stream;
    const bool bwd = q.grads != nullptr, two = c->nl == 2;
    if (bwd && (!q.grads[0] || !q.grads[1] || !q.grads[5] || !q.grads[6] || !q.grads[7] || !q.grads[8] || (two && (!q.grads[2] || !q.grads[3] || !q.grads[4]))))
        FAIL(c, LRCN_EINVAL, "null gradient tensor");
    const DropSpec d1 = make_drop(q.drop, 1), d2 = make_drop(q.drop, 2);
    const DropSpec none{};

    c->cur_B = B;
    const bool epi = !stepwise && lstm_epi_on(c, B) && !lstm_fused_on(c->dt, B, H1, c->ldH1, c->ld4H1);  // (no cell epilogues in the stepwise forward)
    ShadowNeed sh{};
    sh.bwd = bwd; sh.gi = epi;
    r = prepare_weights(c, q.p, sh);
    if (r) return r;
    if (q.lens) {
        if ((r = upload_lens(c, q.lens, B))) return r;
        k_build_tokens_var(st, q.tokens, c->lens_dev, T, B, V, c->tok_in, c->tok_tgt, c->logp);
        if (q.row_w && (r = upload_row_w(c, q.row_w, B))) return r;
    } else {
        k_build_tokens(st, q.tokens, T, B, V, c->tok_in, c->tok_tgt, c->logp);  // reads the caller's (T, B) ids once (T = 0: never)
    }
    // input = input * param[end-3]   lrcn.jl:558.  The two-layer model needs x_cnn only at LSTM-2's input, after the whole first
    // recurrence: its three launches (transpose, split-K GEMM, reduce: ~20 us at 32 rows) run on the weight-gradient stream beside that
    // chain and are joined before the concat (round 5).  Not beside the capped VGG forward from 256 rows (as the weight gradients:
    // there a second stream of LSTM-side workgroups takes CUs from the convolutions); LRCN_WG_STREAM=0 / 1 forces it off / on.
    const bool beside_vgg = !lstm_alone(c) && B >= kBgMinRows;
    const bool par = knob_set("LRCN_WG_STREAM") ? !knob_off("LRCN_WG_STREAM") : !beside_vgg;  // the weight-gradient stream is in use
    const bool xfork = two && par && !stepwise;
    auto image_embedding = [&](hipStream_t s_, bool on_wg) -> int {
        // feats (B x 4096 column-major = memory [4096][B]) -> F [B][4096] (T)
        k_transpose(s_, dt, 1, q.feats, B, LRCN_CNNOUT, B, c->F, LRCN_CNNOUT, 0);
        return gemm(c, dt, c->F, LRCN_CNNOUT, c->Wcd, LRCN_CNNOUT, c->xcnn, c->ldh, B, h, LRCN_CNNOUT, nullptr, true, false, false, false, on_wg);
    };
    if (q.ss) {
        if (!c->sched_cnt) DALLOC(c, c->sched_cnt, 2 * sizeof(long long));
        long long eligible = 0;
        for (int b = 0; b < B; ++b) eligible += q.lens[b];
        k_sched_stats_set(st, c->sched_cnt, stepwise ? 0 : eligible, 0);  // the stepwise route counts its coins on the device
    }
    // Scheduled sampling with eps > 0: step s+1's input is a function of step s's logits, so nothing is time-batched.  Per step, on the rows
    // [s*B, (s+1)*B) of the buffers the time-batched route fills: input projection, one step of LSTM-1, (projection, concat + dropout, input
    // projection, one step of LSTM-2,) the logits GEMM, and the kernel that decides and gathers the input of step s+1.  Every launch applies
    // the dropout multipliers of step s itself: the backward pass regenerates them from (s, b, j).  x_cnn is needed at step 0, so the image
    // embedding runs on the main stream.
    auto sched_forward = [&]() -> int {
        if (int e = image_embedding(st, false)) return e;
        const bool fused1 = lstm_fused_on(dt, B, H1, c->ldH1, c->ld4H1), fused2 = two && lstm_fused_on(dt, B, H2, c->ldH2, c->ld4H2);
        const bool alone = lstm_alone(c);
        const auto rg = rec_gemm(c);
        k_embed_gather(st, dt, c->WeT, c->ldE, c->tok_in, 1, B, E, two ? d1 : none, c->Xemb, c->ldX1);  // step 0: bos
        for (int s = 0; s < S; ++s) {
            const int64_t m0 = (int64_t)s * B;
            void *Xs = boff(c->Xemb, m0 * c->ldX1, es);
            if (!two) k_concat_x2(st, dt, Xs, c->ldX1, c->xcnn, c->ldh, 1, B, E, h, d1, s);
            GEMM(c, dt, Xs, c->ldX1, c->W1x, c->ldX1, c->G1 + m0 * 4 * H1, 4 * H1, B, 4 * H1, X1, q.p[1], true);
            if (int e = lstm_step_fwd(c, alone, rg, fused1, s, B, H1, c->ldH1, c->ld4H1, c->G1, c->W1h, c->A1, c->C1, c->H1all)) return e;
            const void *Hs = boff(c->H1all, m0 * c->ldH1, es);
            if (two) {
                void *X2s = boff(c->X2, m0 * c->ldH2, es);
                GEMM(c, dt, Hs, c->ldH1, c->Wpd, c->ldH1, X2s, c->ldH2, B, h, H1, nullptr, false);
                k_concat_x2(st, dt, X2s, c->ldH2, c->xcnn, c->ldh, 1, B, h, h, d2, s);
                GEMM(c, dt, X2s, c->ldH2, c->W2x, c->ldH2, c->G2 + m0 * 4 * H2, 4 * H2, B, 4 * H2, H2, q.p[3], true);
                if (int e = lstm_step_fwd(c, alone, rg, fused2, s, B, H2, c->ldH2, c->ld4H2, c->G2, c->W2h, c->A2, c->C2, c->H2all)) return e;
                Hs = boff(c->H2all, m0 * c->ldH2, es);
            }
            GEMM(c, dt, Hs, c->ldH2, c->Wod, c->ldH2, c->Logits + m0 * c->ldV, c->ldV, B, V, H2, q.p[8], true);
            if (s + 1 < S) {
                SchedNext a{};
                a.logits = c->Logits + m0 * c->ldV; a.ld_l = c->ldV;
                a.V = V; a.B = B; a.s_next = s + 1;
                a.lens = c->lens_dev;
                a.eps = q.ss->eps; a.temp = q.ss->temperature;
                a.k0 = (uint32_t)q.ss->seed; a.k1 = (uint32_t)(q.ss->seed >> 32);
                a.row0 = (uint32_t)q.ss->row0;
                a.tok_in = c->tok_in;
                a.wembT = c->WeT; a.ld_w = c->ldE; a.E = E;
                a.d = two ? d1 : none;
                a.xemb = c->Xemb; a.ld_x = c->ldX1;
                a.cnt = c->sched_cnt;
                k_sched_next_input(st, dt, a);
            }
        }
        KCHK(c, "stepwise forward");
        return LRCN_OK;
    };
    int rx = LRCN_OK;
    if (stepwise) {
        if ((r = sched_forward())) return r;
    } else if (xfork) {
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
        GEMM(c, dt, c->Xemb, c->ldX1, c->W1x, c->ldX1, c->G1, 4 * H1, M, 4 * H1, X1, q.p[1], true);
        return lstm_layer_fwd(c, S, B, H1, c->ldH1, c->ld4H1, c->G1, c->W1h, c->A1, c->C1, c->H1all, epi ? c->W1h_gi : nullptr);
    };
    if (!stepwise) r = first_layer();
    if (xfork) {  // joined on EVERY exit: the side chain reads the caller's feats
        if (hipStreamWaitEvent(st, c->xc_done, 0) != hipSuccess) (void)hipStreamSynchronize(c->wg_stream);
        if (rx) return rx;
    }
    if (r) return r;
    const void *Htop = two ? c->H2all : c->H1all;  // the hidden states the logits are computed from
    if (two && !stepwise) {
        // x = s[1]*w[end-4]; x = hcat(x, x_cnn); x = dropout(x)    lrcn.jl:544-547
        GEMM(c, dt, c->H1all, c->ldH1, c->Wpd, c->ldH1, c->X2, c->ldH2, M, h, H1, nullptr, false);
        k_concat_x2(st, dt, c->X2, c->ldH2, c->xcnn, c->ldh, S, B, h, h, d2);
        // LSTM 2
        GEMM(c, dt, c->X2, c->ldH2, c->W2x, c->ldH2, c->G2, 4 * H2, M, 4 * H2, H2, q.p[3], true);
        r = lstm_layer_fwd(c, S, B, H2, c->ldH2, c->ld4H2, c->G2, c->W2h, c->A2, c->C2, c->H2all, epi ? c->W2h_gi : nullptr);
        if (r) return r;
    }
    // logits for all steps: x * w[end-1] .+ w[end]   lrcn.jl:550
    if (!stepwise) GEMM(c, dt, Htop, c->ldH2, c->Wod, c->ldH2, c->Logits, c->ldV, M, V, H2, q.p[8], true);
    if (q.fed_out) HIPCHK(c, hipMemcpyAsync(q.fed_out, c->tok_in, sizeof(int32_t) * (size_t)M, hipMemcpyDeviceToDevice, st));
    if (q.logits_out) {  // (T+1) blocks of B x V column-major: block s memory [V][B]
        for (int s = 0; s < S; ++s)
            k_transpose_f32(st, c->Logits + (int64_t)s * B * c->ldV, c->ldV, B, V, q.logits_out + (int64_t)s * B * V, B);
    }
    const float scale = (float)(1.0 / (q.lens ? (double)q.norm_tokens : (double)q.norm_B * (double)S));
    if (c->opt_det && !c->logp_rows) DALLOC(c, c->logp_rows, sizeof(double) * (size_t)c->maxS * c->maxB);
    XentCall x{};
    x.logits = c->Logits; x.ld_l = c->ldV; x.tgt = c->tok_tgt; x.M = M; x.V = V; x.scale = scale;
    x.dlog = bwd ? c->dLog : nullptr; x.ld_d = c->ldV;
    x.sum = c->logp; x.rows = c->opt_det ? c->logp_rows : nullptr;
    x.masked = q.lens != nullptr; x.row_w = q.row_w ? c->roww_dev : nullptr; x.B = B; x.eps = q.smooth;
    if (q.smooth > 0.0f) {  // label smoothing: the plain terms go to a second accumulator (lrcn_smooth_stats)
        if (!c->nll_acc) DALLOC(c, c->nll_acc, sizeof(double));
        if (x.rows && !c->ll_rows) DALLOC(c, c->ll_rows, sizeof(double) * (size_t)c->maxS * c->maxB);
        HIPCHK(c, hipMemsetAsync(c->nll_acc, 0, sizeof(double), st));
        x.ll_sum = c->nll_acc; x.ll_rows = x.rows ? c->ll_rows : nullptr;
    }
    k_softmax_xent(st, dt, x);
    c->last_norm = q.norm_B;
    c->last_S = S;
    c->last_tokens = q.lens ? q.norm_tokens : 0;
    KCHK(c, "forward");
    if (!bwd) return LRCN_OK;

    const int64_t ldM = ld64(M), ldB = ld64(B);
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
    // One layer's weight and bias gradient, on sw.  The contraction runs over the M = S*B rows, so its operands are materialised transposed
    // (K-contiguous) by one launch: dY (T) [M][ldY], NY columns, into TA; the layer's input x (T) [M][ldx], X columns, into TB, and for an
    // LSTM the previous step's hidden state (Hprev, Hp columns; NULL: none) stacked below it, so that dW [NY][X + Hp] = dY' [x | h_prev] is
    // ONE GEMM.  db (NULL: the layer has no bias) = the column sums of dY.
    auto weight_grad = [&](const void *dY, int64_t ldY, int NY, const void *x, int64_t ldx, int X, const void *Hprev, int64_t ldHp, int Hp,
                           float *dW, float *db) -> int {
        TrPlan pl{};
        auto tr = [&](const void *src, int64_t ld_src, int R, int C, void *dst, int shift) {
            TrDesc &d = pl.d[pl.n++];
            d.src = src; d.ld_src = ld_src; d.R = R; d.C = C; d.dst = dst; d.ld_dst = ldM; d.shift = shift;
        };
        tr(dY, ldY, M, NY, c->TA, 0);   // dY^T [NY][ldM]
        tr(x, ldx, M, X, c->TB, 0);     // x^T [X][ldM]
        if (Hprev) tr(Hprev, ldHp, M - B, Hp, boff(c->TB, (int64_t)X * ldM, es), M > B ? B : 0);  // h_prev^T [Hp][ldM] (one step later)
        k_transpose_multi(sw, dt, pl);
        const int Xh = X + (Hprev ? Hp : 0);
        GEMM(c, dt, c->TA, ldM, c->TB, ldM, dW, Xh, NY, Xh, M, nullptr, true, false, false, false, par);
        if (db) k_colsum(sw, dt, dY, ldY, M, NY, db, c->opt_det);
        return LRCN_OK;
    };
    // dWcnn = d x_cnn' feats on sw, the last tensor of group 2 in either model
    auto image_embedding_grad = [&]() -> int {
        k_transpose(sw, dt, 1, c->dxcnn, c->ldh, B, h, c->dxcT, ldB, 0);     // dxcnn^T [h][ldB]
        k_cast_rows(sw, dt, q.feats, B, LRCN_CNNOUT, B, c->FT, ldB);           // feats^T [4096][ldB] (it already is, in memory)
        GEMM(c, dt, c->dxcT, ldB, c->FT, ldB, q.grads[5], LRCN_CNNOUT, h, LRCN_CNNOUT, B, nullptr, true, false, false, false, par);
        HIPCHK(c, hipEventRecord(c->grad_ev[2], sw));  // group 2: (Wproj,) Wcnn
        return LRCN_OK;
    };
    // Everything from the first fork on runs inside one scope whose every exit -- the normal one and each early error return --
    // is followed by the join below: an error after a fork must not leave the weight-gradient stream writing the caller's grads[]
    // (and reading the caller's feats) after the call has returned.
    auto backward = [&]() -> int {
    // ---- logits layer: dWout, dbout (sw) | dH2 (main) ----
        if (int e = fork()) return e;
        if (int e = weight_grad(c->dLog, c->ldV, V, Htop, c->ldH2, H2, nullptr, 0, 0, q.grads[7], q.grads[8])) return e;
        HIPCHK(c, hipEventRecord(c->grad_ev[0], sw));  // group 0: Wout, bout
        GEMM(c, dt, c->dLog, c->ldV, c->WoT, c->ldV, two ? c->dH2all : c->dH1all, H2, M, H2, V, nullptr, true);
        if (two) {
            // ---- LSTM 2 ----
            if (int e = lstm_layer_bwd(c, S, B, H2, c->ld4H2, c->A2, c->C2, c->dH2all, c->W2hT, c->dZ2)) return e;
            if (int e = fork()) return e;
            if (int e = weight_grad(c->dZ2, c->ld4H2, 4 * H2, c->X2, c->ldH2, H2, c->H2all, c->ldH2, H2, q.grads[2], q.grads[3])) return e;
        }
        HIPCHK(c, hipEventRecord(c->grad_ev[1], sw));  // group 1: W2, b2
        if (two) {
            GEMM(c, dt, c->dZ2, c->ld4H2, c->W2xT, c->ld4H2, c->dX2, c->ldH2, M, H2, 4 * H2, nullptr, false);
            k_dx2_mask_reduce(st, dt, c->dX2, c->ldH2, S, B, h, h, d2, c->dxcnn, c->ldh);
            // ---- projection and image embedding: dWproj, dWcnn (sw) | dH1 (main) ----
            if (int e = fork()) return e;
            if (int e = weight_grad(c->dX2, c->ldH2, h, c->H1all, c->ldH1, H1, nullptr, 0, 0, q.grads[4], nullptr)) return e;
            GEMM(c, dt, c->dX2, c->ldH2, c->WpT, c->ldh, c->dH1all, H1, M, H1, h, nullptr, true);
            if (int e = image_embedding_grad()) return e;
        }
        // ---- LSTM 1 ----
        if (int e = lstm_layer_bwd(c, S, B, H1, c->ld4H1, c->A1, c->C1, c->dH1all, c->W1hT, c->dZ1)) return e;
        if (int e = fork()) return e;
        if (int e = weight_grad(c->dZ1, c->ld4H1, 4 * H1, c->Xemb, c->ldX1, X1, c->H1all, c->ldH1, H1, q.grads[0], q.grads[1])) return e;
        HIPCHK(c, hipEventRecord(c->grad_ev[3], sw));  // group 3: W1, b1
        GEMM(c, dt, c->dZ1, c->ld4H1, c->W1xT, c->ld4H1, c->dXemb, c->ldX1, M, X1, 4 * H1, nullptr, true);
        if (!two) {
            // LRCN-1f: d[embedding | x_cnn] -- mask all E + h columns in place, sum the right h columns over the steps -> d x_cnn,
            // then the image-embedding gradient exactly as in the two-layer model (on sw, after the dW1 GEMM that shares its scratch)
            k_dx2_mask_reduce(st, GEMM_T_F32, c->dXemb, c->ldX1, S, B, E, h, d1, c->dxcnn, c->ldh);
            if (int e = fork()) return e;
            if (int e = image_embedding_grad()) return e;
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
            if (!k_embed_scatter_rm(st, c->dXemb, c->ldX1, c->tok_in, S, B, E, V, two ? d1 : none, c->dWe_rm, c->ldE, q.grads[6], keys))
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
    KCHK(c, "backward");
    return LRCN_OK;
}

// logp[0] = running sum of log p(target); logp[1] = sticky "token id outside [0, V)" flag raised by build_tokens_kernel
int lrcn_impl::fetch_loss(lrcn_ctx *c, double *out) {
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

namespace {

// The body of the lrcn_loss* entry points: q.form says which of lens / row_w / ss the entry point requires (the others it leaves NULL, but
// for the scheduled-sampling form's optional row_w); q.grads NULL: the loss alone.
int loss_entry(lrcn_ctx *c, const LossCall &q, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !q.p || !q.feats || (!q.tokens && q.T > 0)) return LRCN_EINVAL;
    if (q.form != LossCall::PLAIN && !q.lens) FAIL(c, LRCN_EINVAL, "lens is NULL");
    if (q.form == LossCall::WEIGHTED && !q.row_w) FAIL(c, LRCN_EINVAL, "row_w is NULL");
    if (q.form == LossCall::SCHED && !q.ss) FAIL(c, LRCN_EINVAL, "the lrcn_sched argument is NULL");
    int r = loss_impl(c, q);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

// The body of the lrcn_train_step* entry points: lossgradient (q, whose p is set here and whose grads the entry point sets), then update! --
// with max_norm > 0 on the gradient clipped to that global norm (the nine sums of squares, norm / scale / skip and the clipped update, all
// on the context's stream).
int train_step_impl(lrcn_ctx *c, LossCall q, float *const p[9], float *const m[9], float *const v[9], int step, float lr, float b1, float b2,
                    float eps, float max_norm, double *loss_host) {
    DeviceGuard dg(c);
    if (!c || !p || !q.grads || !m || !v) return LRCN_EINVAL;
    if (std::isnan(max_norm)) FAIL(c, LRCN_EINVAL, "max_norm is NaN");
    const bool clip = max_norm > 0.0f;
    if (clip && step < 1) return LRCN_EINVAL;  // (the unclipped step finds a bad `step` in its update, after the pass)
    q.p = p;
    int r = loss_entry(c, q, nullptr);
    if (r) return r;
    if (clip) {
        r = lrcn_grad_sumsq_model(c, q.grads, -1, nullptr);
        if (r || (r = lrcn_clip_set(c, LRCN_CLIP_SLOTS, max_norm, nullptr))) return r;
    } else if (step < 1) {
        return LRCN_EINVAL;
    }
    r = adam_update(c, p, q.grads, m, v, step, lr, b1, b2, eps, clip);
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

}  // namespace

extern "C" {

int lrcn_loss(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, int norm_B,
              const lrcn_dropout *drop, double *loss_host) {
    LossCall q{};
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.norm_B = norm_B; q.drop = drop;
    return loss_entry(c, q, loss_host);
}

int lrcn_loss_grad(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, int norm_B,
                   const lrcn_dropout *drop, float *const grads[9], double *loss_host) {
    if (!grads) return LRCN_EINVAL;
    LossCall q{};
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.norm_B = norm_B; q.drop = drop; q.grads = grads;
    return loss_entry(c, q, loss_host);
}

// ---- include/lrcn_varlen.h: per-row caption lengths ----
int lrcn_loss_var(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B,
                  int64_t norm_tokens, const lrcn_dropout *drop, double *loss_host) {
    LossCall q{};
    q.form = LossCall::VAR; q.lens = lens; q.norm_tokens = norm_tokens;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop;
    return loss_entry(c, q, loss_host);
}

int lrcn_loss_grad_var(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B,
                       int64_t norm_tokens, const lrcn_dropout *drop, float *const grads[9], double *loss_host) {
    if (!grads) return LRCN_EINVAL;
    LossCall q{};
    q.form = LossCall::VAR; q.lens = lens; q.norm_tokens = norm_tokens;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = grads;
    return loss_entry(c, q, loss_host);
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
    LossCall q{};
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.norm_B = B; q.logits_out = logits_out;
    return loss_impl(c, q);
}

int lrcn_avg_loss_batch(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, int T, int B, double *loss_host) {
    // average_loss's loop body (lrcn.jl:452-475): pdrop 0, normalised by the batch's own size (lrcn.jl:412)
    LossCall q{};
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.norm_B = B;
    return loss_entry(c, q, loss_host);
}

int lrcn_train_step(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                    const int32_t *tokens, int T, int B, int norm_B, const lrcn_dropout *drop, int step, float lr, float b1,
                    float b2, float eps, double *loss_host) {
    return lrcn_train_step_clip(c, p, g, m, v, feats, tokens, T, B, norm_B, drop, step, lr, b1, b2, eps, /* max_norm */ 0.0f, loss_host);
}

int lrcn_train_step_var(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                        const int32_t *tokens, const int32_t *lens, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, int step,
                        float lr, float b1, float b2, float eps, double *loss_host) {
    return lrcn_train_step_var_clip(c, p, g, m, v, feats, tokens, lens, T, B, norm_tokens, drop, step, lr, b1, b2, eps, /* max_norm */ 0.0f, loss_host);
}

// ---- include/lrcn_clip.h: max_norm <= 0 is the unclipped step ----
int lrcn_train_step_clip(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                         const int32_t *tokens, int T, int B, int norm_B, const lrcn_dropout *drop, int step, float lr, float b1, float b2,
                         float eps, float max_norm, double *loss_host) {
    LossCall q{};
    q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.norm_B = norm_B; q.drop = drop; q.grads = g;
    return train_step_impl(c, q, p, m, v, step, lr, b1, b2, eps, max_norm, loss_host);
}

int lrcn_train_step_var_clip(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                             const int32_t *tokens, const int32_t *lens, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop,
                             int step, float lr, float b1, float b2, float eps, float max_norm, double *loss_host) {
    LossCall q{};
    q.form = LossCall::VAR; q.lens = lens; q.norm_tokens = norm_tokens;
    q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = g;
    return train_step_impl(c, q, p, m, v, step, lr, b1, b2, eps, max_norm, loss_host);
}

// ---- include/lrcn_weighted.h: a real weight per caption row ----
int lrcn_loss_w(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, const float *row_w,
                int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, double *loss_host) {
    LossCall q{};
    q.form = LossCall::WEIGHTED; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop;
    return loss_entry(c, q, loss_host);
}

int lrcn_loss_grad_w(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                     const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, float *const grads[9],
                     double *loss_host) {
    if (!grads) return LRCN_EINVAL;
    LossCall q{};
    q.form = LossCall::WEIGHTED; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = grads;
    return loss_entry(c, q, loss_host);
}

int lrcn_train_step_w(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                      const int32_t *tokens, const int32_t *lens, const float *row_w, int T, int B, int64_t norm_tokens,
                      const lrcn_dropout *drop, int step, float lr, float b1, float b2, float eps, float max_norm, double *loss_host) {
    LossCall q{};
    q.form = LossCall::WEIGHTED; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens;
    q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = g;
    return train_step_impl(c, q, p, m, v, step, lr, b1, b2, eps, max_norm, loss_host);
}

// ---- include/lrcn_sched.h: scheduled sampling (row_w optional) ----
int lrcn_loss_sched(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, const float *row_w,
                    int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss, int32_t *fed_out, float *logits_out,
                    double *loss_host) {
    LossCall q{};
    q.form = LossCall::SCHED; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens; q.ss = ss; q.fed_out = fed_out; q.logits_out = logits_out;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop;
    return loss_entry(c, q, loss_host);
}

int lrcn_loss_grad_sched(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                         const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss,
                         float *const grads[9], int32_t *fed_out, float *logits_out, double *loss_host) {
    if (!grads) return LRCN_EINVAL;
    LossCall q{};
    q.form = LossCall::SCHED; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens; q.ss = ss; q.fed_out = fed_out; q.logits_out = logits_out;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = grads;
    return loss_entry(c, q, loss_host);
}

int lrcn_train_step_sched(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                          const int32_t *tokens, const int32_t *lens, const float *row_w, int T, int B, int64_t norm_tokens,
                          const lrcn_dropout *drop, const lrcn_sched *ss, int step, float lr, float b1, float b2, float eps, float max_norm,
                          double *loss_host) {
    LossCall q{};
    q.form = LossCall::SCHED; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens; q.ss = ss;
    q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = g;
    return train_step_impl(c, q, p, m, v, step, lr, b1, b2, eps, max_norm, loss_host);
}

int lrcn_sched_stats(lrcn_ctx *c, int64_t *eligible, int64_t *drawn) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    long long n[2] = {0, 0};
    if (c->sched_cnt) HIPCHK(c, hipMemcpyAsync(n, c->sched_cnt, sizeof(n), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (eligible) *eligible = n[0];
    if (drawn) *drawn = n[1];
    return LRCN_OK;
}

// ---- include/lrcn_smooth.h: label smoothing (row_w and ss optional) ----
namespace {
// the LossCall of a *_smooth entry point: the padded batch with whichever of row_w / ss is given; smooth is checked before any GPU work
int smooth_call(lrcn_ctx *c, LossCall &q, const int32_t *lens, const float *row_w, int64_t norm_tokens, const lrcn_sched *ss, float smooth) {
    if (!c) return LRCN_EINVAL;
    if (!(smooth >= 0.0f && smooth <= 1.0f)) FAIL(c, LRCN_EINVAL, "smooth=%g outside [0,1]", (double)smooth);
    q.form = LossCall::VAR; q.lens = lens; q.row_w = row_w; q.norm_tokens = norm_tokens; q.ss = ss; q.smooth = smooth;
    return LRCN_OK;
}
}  // namespace

int lrcn_loss_smooth(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens, const float *row_w,
                     int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss, int32_t *fed_out, float smooth,
                     double *loss_host) {
    LossCall q{};
    if (int r = smooth_call(c, q, lens, row_w, norm_tokens, ss, smooth)) return r;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.fed_out = fed_out;
    const int r = loss_entry(c, q, loss_host);
    if (!r) c->last_smooth = smooth;
    return r;
}

int lrcn_loss_grad_smooth(lrcn_ctx *c, const float *const p[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                          const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss,
                          int32_t *fed_out, float smooth, float *const grads[9], double *loss_host) {
    if (!grads) return LRCN_EINVAL;
    LossCall q{};
    if (int r = smooth_call(c, q, lens, row_w, norm_tokens, ss, smooth)) return r;
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.fed_out = fed_out; q.grads = grads;
    const int r = loss_entry(c, q, loss_host);
    if (!r) c->last_smooth = smooth;
    return r;
}

int lrcn_train_step_smooth(lrcn_ctx *c, float *const p[9], float *const g[9], float *const m[9], float *const v[9], const float *feats,
                           const int32_t *tokens, const int32_t *lens, const float *row_w, int T, int B, int64_t norm_tokens,
                           const lrcn_dropout *drop, const lrcn_sched *ss, float smooth, int step, float lr, float b1, float b2, float eps,
                           float max_norm, double *loss_host) {
    LossCall q{};
    if (int r = smooth_call(c, q, lens, row_w, norm_tokens, ss, smooth)) return r;
    q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.drop = drop; q.grads = g;
    const int r = train_step_impl(c, q, p, m, v, step, lr, b1, b2, eps, max_norm, loss_host);
    if (!r) c->last_smooth = smooth;
    return r;
}

int lrcn_smooth_stats(lrcn_ctx *c, double *nll, double *smoothed) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (c->last_smooth < 0.0f) FAIL(c, LRCN_ESTATE, "lrcn_smooth_stats: the context has made no *_smooth call");
    double s = 0.0, n = 0.0;
    HIPCHK(c, hipMemcpyAsync(&s, c->logp, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (c->last_smooth > 0.0f) HIPCHK(c, hipMemcpyAsync(&n, c->nll_acc, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double norm = c->last_tokens > 0 ? (double)c->last_tokens : (double)c->last_norm * (double)c->last_S;
    if (smoothed) *smoothed = -s / norm;
    if (nll) *nll = -(c->last_smooth > 0.0f ? n : s) / norm;
    return LRCN_OK;
}

int lrcn_xent_logits(lrcn_ctx *c, const float *logits, int64_t ld, const int32_t *tgt, const float *row_w, int M, int B, int V, float scale,
                     float smooth, int out_dtype, void *dlog, int64_t ld_d, double *terms, double *ll_terms) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (!logits || !tgt) FAIL(c, LRCN_EINVAL, "null argument");
    if (M < 1 || B < 1 || V < 1 || ld < V) FAIL(c, LRCN_EINVAL, "M=%d, B=%d, V=%d must be >= 1 and ld=%lld >= V", M, B, V, (long long)ld);
    if (dlog && ld_d < V) FAIL(c, LRCN_EINVAL, "ld_d=%lld must be >= V=%d", (long long)ld_d, V);
    if (out_dtype != LRCN_F32 && out_dtype != LRCN_BF16) FAIL(c, LRCN_EINVAL, "out_dtype=%d is neither LRCN_F32 nor LRCN_BF16", out_dtype);
    if (!std::isfinite(scale)) FAIL(c, LRCN_EINVAL, "scale=%g is not finite", (double)scale);
    if (!(smooth >= 0.0f && smooth <= 1.0f)) FAIL(c, LRCN_EINVAL, "smooth=%g outside [0,1]", (double)smooth);
    hipStream_t st = c->stream;
    // scratch: M doubles (the row terms of the unsmoothed kernels when the caller wants none) and the M checked targets
    const size_t need = (sizeof(double) + sizeof(int32_t)) * (size_t)M;
    if (need > c->xl_bytes) {
        HIPCHK(c, hipStreamSynchronize(st));  // an earlier call's launches may still read the old one
        if (c->xl_arena) (void)hipFree(c->xl_arena);
        c->xl_arena = nullptr;
        c->xl_bytes = 0;
        if (hipMalloc(&c->xl_arena, 2 * need) != hipSuccess) FAIL(c, LRCN_ENOMEM, "hipMalloc(%zu) for lrcn_xent_logits failed", 2 * need);
        c->xl_bytes = 2 * need;
    }
    double *rows_scratch = reinterpret_cast<double *>(c->xl_arena);
    int32_t *tg = reinterpret_cast<int32_t *>(rows_scratch + M);
    k_xent_targets(st, tgt, M, V, tg);
    const int dt = out_dtype == LRCN_BF16 ? GEMM_T_BF16 : GEMM_T_F32;
    const bool sm = smooth > 0.0f;  // the unsmoothed kernels write one set of terms, and need a place for it
    XentCall x{};
    x.logits = logits; x.ld_l = ld; x.tgt = tg; x.M = M; x.V = V; x.scale = scale; x.dlog = dlog; x.ld_d = ld_d;
    x.rows = (sm || terms) ? terms : ll_terms ? ll_terms : rows_scratch;
    x.masked = true; x.row_w = row_w; x.B = B; x.eps = smooth; x.ll_rows = sm ? ll_terms : nullptr;
    k_softmax_xent(st, dt, x);
    if (!sm && terms && ll_terms) HIPCHK(c, hipMemcpyAsync(ll_terms, terms, sizeof(double) * (size_t)M, hipMemcpyDeviceToDevice, st));
    KCHK(c, "xent_logits");
    return LRCN_OK;
}

}  // extern "C"
