// ctx.h -- the caption model's context (struct lrcn_ctx, opaque at the ABI) and the internal helpers that more than one of its
// files needs: lrcn_api.hip (context, GEMM helper, single step), train.hip (forward / backward pass, loss and train-step entry points),
// update.hip (shadow weights, Adam, gradient-norm clipping), train_dp.hip (data parallelism), decode.hip (beam search, sampling, n-best,
// scoring), vgg.hip (VGG-16 forward).
#pragma once
#include <utility>

#include "comm.h"
#include "host.h"
#include "../../include/lrcn_smooth.h"

namespace lrcn_impl {

struct VggLayer {
    void *w = nullptr;    // [Cout][9*Cin] T (conv) ; conv1_1: [64][32]
    void *w_fused = nullptr;  // conv1_1 only (bf16): [64][32] in the K order of the fused conv1_1+conv1_2 kernel
    float *b = nullptr;   // [Cout] f32
    int Cin = 0, Cout = 0, S = 0, pool = 0;
    // LRCN_FP8 (layers conv2_2 .. conv5_3): e4m3 weights [Cout][9*Cin], per-channel weight scale, effective epilogue scale/bias
    void *w8 = nullptr;
    float *sw = nullptr, *escale = nullptr, *ebias = nullptr;
};
constexpr int kFp8First = 3;  // conv2_2: the first layer with Cin % 128 == 0

}  // namespace lrcn_impl

struct lrcn_ctx {
    lrcn_config cfg{};
    hipStream_t stream = nullptr;
    std::string err;
    std::vector<void *> allocs;
    int dt = 0, vdt = 0;
    size_t esz = 4, vesz = 4;
    int E = 0, H1 = 0, H2 = 0, h = 0, V = 0, maxB = 0, maxS = 0;
    int nl = 2;             // LSTM layers: 2 = the reference's LRCN-2f (lrcn.jl:540-551), 1 = LRCN-1f (BASELINE configs[1])
    int X1 = 0;             // input width of LSTM-1: E (2 layers) or E + h = [embedding | x_cnn] (1 layer)
    int64_t ldX1 = 0;
    int64_t ldE = 0, ldH1 = 0, ldH2 = 0, ldh = 0, ld4H1 = 0, ld4H2 = 0, ldV = 0, ldM = 0, ldB = 0;
    // shadow weights (T)
    void *W1x = nullptr, *W1h = nullptr, *W1xT = nullptr, *W1hT = nullptr;
    // decode only: [x | h] concatenated along K -- weights [4H][ldXH] and the step inputs [B][ldXH]: one gate GEMM per LSTM
    void *W1cat = nullptr, *W2cat = nullptr, *st_xh1 = nullptr, *st_xh2 = nullptr;
    int64_t ldXH1 = 0, ldXH2 = 0;
    void *W2x = nullptr, *W2h = nullptr, *W2xT = nullptr, *W2hT = nullptr;
    // batched decode with input-projection TABLES (round 6; decode_tables_on): T1 [V][4H1] = Wembed W1x + b1 per TOKEN, U2 [images][4H2] =
    // x_cnn W2x(right half) + b2 per IMAGE (f32, gate-block columns), the gate GEMMs' operands A1 = h1[parent] and A2 = [h1 Wproj | h2[parent]],
    // W2's matching weights (x_cnn columns left out, rows interleaved) and the image of every hypothesis row; all lazily allocated
    float *dec_T1 = nullptr, *dec_U2 = nullptr;
    void *dec_A1 = nullptr, *dec_A2 = nullptr, *dec_W2c = nullptr, *dec_Aimg = nullptr;
    int32_t *dec_img = nullptr;
    float *smax_part = nullptr;             // [maxB][2 ceil(V / 256)][SMAX_REC]: the logits GEMM's softmax / top-K records of a batched decode step (round 6), lazily
    void *alt_gi[2] = {nullptr, nullptr};   // LRCN_OPT_FUSED_UPDATE: the second set's gate-interleaved copies (round 6), written by the Adam kernel
    bool gi_live = false;                   // a training call has taken the cell-epilogue route: the fused update keeps the interleaved copies current
    bool shadow_has_gi = false;             // ... and the current set's were made by it
    void *W1h_gi = nullptr, *W2h_gi = nullptr;  // recurrent weights with (unit, gate)-interleaved rows (gemm_8p.hip LSTM_FWD epilogue), lazily
    void *Wpd = nullptr, *WpT = nullptr, *Wcd = nullptr, *WeT = nullptr, *Wod = nullptr, *WoT = nullptr;
    // LRCN_OPT_FUSED_UPDATE: the second set of the 14 training shadows above.  The Adam kernel of a train step writes the NEXT step's
    // shadows into it while (per-group pipeline) the backward pass may still be reading the current set; then the two sets swap roles.
    void *alt[14] = {};
    bool opt_fused = false, opt_det = false;
    int64_t conv_chunk_bytes = 0;           // LRCN_OPT_CONV_CHUNK_BYTES (0 = default)
    unsigned fused_groups = 0;              // gradient groups whose fused Adam has been issued in the current step (bit per group)
    int fused_step = 0;                     // the `step` those bits belong to: a call with another step starts a new mask
    unsigned refresh_groups = 0;            // lrcn_refresh_shadows_group: groups whose shadows of the NEXT step have been issued
    // gradient-norm clipping (include/lrcn_clip.h), lazily: the control block and k_sumsq's partial sums [9][kSumsqParts], one slice per slot
    struct ClipCtl *clip_ctl = nullptr;
    double *clip_parts = nullptr;
    bool shadow_valid = false;              // the current set holds the shadows (direct AND transposed) of the parameters at shadow_p
    const float *shadow_p[9] = {};
    float *dWe_rm = nullptr;                // [V][ldE] f32, all zero between calls: row-major staging of the embedding gradient
    unsigned long long *sort_keys = nullptr;  // [maxS * maxB] (token, row) keys of the ordered embedding-gradient sums
    double *logp_rows = nullptr;            // [maxS * maxB] per-row log p(target): the ordered loss sum of LRCN_OPT_DETERMINISTIC
    // sparse exchange of the embedding gradient (lrcn_set_embed_rows_buffer): lossgradient writes its (T+1) B rows of d(x_lstm) and their
    // token ids HERE instead of scattering them into the dense gradient; lrcn_embed_grad_from_rows sums the rows of all ranks in a fixed order
    float *emb_rows_out = nullptr;
    int32_t *emb_tok_out = nullptr;
    int emb_rows_cap = 0;
    unsigned long long *imp_keys = nullptr;  // [8192] sort keys of lrcn_embed_grad_from_rows
    // activations
    int32_t *tok = nullptr, *tok_in = nullptr, *tok_tgt = nullptr;
    void *F = nullptr, *FT = nullptr;
    float *xcnn = nullptr;
    void *Xemb = nullptr, *A1 = nullptr, *H1all = nullptr, *X2 = nullptr, *A2 = nullptr, *H2all = nullptr;
    float *G1 = nullptr, *C1 = nullptr, *G2 = nullptr, *C2 = nullptr, *Logits = nullptr;
    void *dLog = nullptr, *dZ1 = nullptr, *dZ2 = nullptr, *dX2 = nullptr;
    float *dH1all = nullptr, *dH2all = nullptr, *dXemb = nullptr, *dhrec = nullptr, *dc = nullptr, *dxcnn = nullptr;
    void *TA = nullptr, *TB = nullptr;  // transposed-operand scratch: up to [max(4H,V)][ldM] and [max(2*H2, E+H1)][ldM]
    void *dxcT = nullptr;
    double *logp = nullptr;
    void *zero_page = nullptr;
    hipEvent_t grad_ev[LRCN_GRAD_GROUPS] = {};  // recorded when the gradients of a group are final (lrcn_grad_group_wait)
    void *gemm_ws = nullptr;  // split-K slabs of gemm_8p / gemm_skinny (LSTM side)
    void *vgg_ws = nullptr;   // same for fc6/fc7: the VGG forward may run on another stream, concurrently with the LSTM step
    size_t gemm_ws_bytes = 0;
    int last_norm = 1, last_S = 1;
    int64_t last_tokens = 0;  // > 0: the last loss call was a variable-length one (include/lrcn_varlen.h) and this is its norm_tokens
    // per-row lengths of the variable-length entry points: device [maxB], uploaded through kLenSlots pinned slots [maxB] each, used in
    // turn (a slot is rewritten once the upload that last read it has run: the host may queue kLenSlots steps ahead of the device)
    static constexpr int kLenSlots = 4;
    int32_t *lens_dev = nullptr, *lens_pin = nullptr;
    hipEvent_t lens_up[kLenSlots] = {};
    int lens_slot = 0;
    // per-row loss weights of include/lrcn_weighted.h: device f32 [maxB], uploaded as the lengths are, through a slot ring of their own
    float *roww_dev = nullptr, *roww_pin = nullptr;
    hipEvent_t roww_up[kLenSlots] = {};
    int roww_slot = 0;
    // include/lrcn_smooth.h, lazily: the second accumulator of a label-smoothed call (the sum of the plain log-likelihood terms), its per-row
    // slots [maxS * maxB] under LRCN_OPT_DETERMINISTIC, and lrcn_xent_logits' scratch (checked targets, row terms nobody asked for)
    double *nll_acc = nullptr, *ll_rows = nullptr;
    float last_smooth = -1.0f;       // the smooth of the most recent *_smooth call (< 0: there has been none)
    void *xl_arena = nullptr;
    size_t xl_bytes = 0;
    long long *sched_cnt = nullptr;  // include/lrcn_sched.h, lazily: {coins taken, coins fired} of the most recent scheduled-sampling call
    int cur_B = 0;  // rows of the loss / lossgradient call in flight (gemm() picks its "beside the convolutions" hint by it)
    // single-step scratch (lrcn_lstm / lrcn_step / beam search), row-major
    float *st_f32[4] = {nullptr, nullptr, nullptr, nullptr};   // h1,c1,h2,c2 [B][H]
    // the other buffer of each state pair: the target of the single-image beam's gather and of the batched decode's k_gather_state, and
    // the c(t) output of the batched decode's cell epilogues (decode_step swaps the pairs after a step)
    float *st2_f32[4] = {nullptr, nullptr, nullptr, nullptr};
    void *st_h1 = nullptr, *st_h2 = nullptr, *st_x = nullptr, *st_x2 = nullptr, *st_a = nullptr;
    float *st_g = nullptr, *st_logits = nullptr, *st_prob = nullptr, *st_io = nullptr, *st_topv = nullptr;
    int32_t *st_topi = nullptr, *st_parent = nullptr;
    // the batched decode (decode_begin / decode_step; lrcn_beam_search_batch and lrcn_sample_batch): token histories (ping-pong for the
    // beam's reorder; the sampler's rows keep bs_seq[0]), next input tokens, done flags and counter, results -- all on the device.  The
    // sampler keeps its lengths in bs_res_len and its log-likelihoods in bs_p; bs_res_tok / bs_res_p are the beams' (the n-best beam's
    // results: [N*K] entries in bs_res_tok / bs_res_len / bs_res_p, scores in nb_res_score)
    int32_t *bs_seq[2] = {nullptr, nullptr}, *bs_last = nullptr, *bs_done = nullptr, *bs_ndone = nullptr, *bs_res_tok = nullptr,
            *bs_res_len = nullptr;
    float *bs_p = nullptr, *bs_res_p = nullptr;
    int32_t *smp_count = nullptr;   // lrcn_sample_batch_p (include/lrcn_nucleus.h), lazily: the admitted-set sizes [maxB][LRCN_BEAM_MAXLEN - 1]
    // lrcn_beam_nbest_batch (include/lrcn_nbest.h), lazily on its first call: the pool's token storage [maxB][2][LRCN_BEAM_MAXLEN] (2K rows per
    // image), the pool [maxB] {score, logp, storage row, length}, per image {live slots, pool count, done}, live cum [maxB], scores out
    int32_t *nb_store = nullptr;
    int4 *nb_pool = nullptr, *nb_img = nullptr;
    float *nb_cum = nullptr, *nb_res_score = nullptr;
    int32_t *dv_done = nullptr;   // lrcn_beam_diverse_batch (include/lrcn_diverse.h), lazily: one done flag per image [maxB]; the rest is nb_*
    // include/lrcn_constrain.h: the call's static ban bitmap [(V + 31) / 32] words, and behind it lrcn_constrained_topk_logits' scratch of
    // the general form (V > 16384); one device buffer, grown to the largest call's need, freed by lrcn_destroy
    void *cn_arena = nullptr;
    size_t cn_bytes = 0;
    // include/lrcn_forced.h, lazily on the first forced call: a step's move values [maxB][LRCN_FORCED_MAXSETS * LRCN_FORCED_MAXALT] and row
    // states [maxB].  The call's word table rides in cn_arena behind the bitmap; the done flags are dv_done, the rest is nb_*.
    float *fc_move = nullptr;
    int32_t *fc_state = nullptr;
    float *ens_mix = nullptr;   // include/lrcn_ensemble.h, lazily on a leader's first call: the mixture rows [maxB][ldV]
    // lrcn_score_matrix / lrcn_score_pairs: one device arena, grown to the largest call's need (include/lrcn_score.h), freed by lrcn_destroy
    void *sc_arena = nullptr;
    size_t sc_bytes = 0;
    // VGG
    int ncu = 0;         // compute units of cfg.device (lrcn_create)
    int vgg_wg_cap = 0;  // > 0: cap on the convolution grids (lrcn_vgg_set_wg_cap)
    bool vgg_loaded = false;
    bool vgg_fp8 = false, fp8_ready = false;  // LRCN_FP8: conv2_2..conv5_3 in e4m3 once lrcn_vgg_calibrate has run
    float *amax_dev = nullptr;                // [13] per-layer output amax collected by the calibration pass
    float act_scale[13] = {};                 // sa of layer l's output (l = 2..12)
    lrcn_impl::VggLayer conv[13];
    void *fc6w = nullptr, *fc7w = nullptr;
    float *fc6b = nullptr, *fc7b = nullptr;
    void *actA = nullptr, *actB = nullptr, *im2col = nullptr, *f6 = nullptr, *img16 = nullptr;
    float *featsRM = nullptr;  // [N][4096] f32 row-major
    // live timing of the dominant kernel (the 12 implicit-GEMM conv launches conv1_2..conv5_3), see lrcn_profile*
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
    size_t prof_used = 0;
    double prof_ms = 0.0;
    int64_t prof_launches = 0;
    // level 2 (lrcn_profile(ctx, 2)): event pairs around the HBM-bound segments of SURVEY 8(d), see lrcn_profile_segment
    int prof_level = 0;
    struct SegProf {
        std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
        size_t used = 0;
        double ms = 0.0, bytes = 0.0;
        int64_t n = 0;
    } seg[LRCN_SEG_COUNT];
    std::string vgg_routes;  // kernel family per layer of the most recent VGG forward (lrcn_debug_route)
    // image front end: the full averageImage (lrcn_set_average_image), per-batch image descriptors, float scratch of the unfused path
    float *avg_img = nullptr;
    bool avg_on = false;
    void *img_meta = nullptr;
    int img_meta_cap = 0;
    float *pre_f32 = nullptr;
    // data parallelism: RCCL communicator (lrcn_comm_init) and one stream per gradient group for [all-reduce -> Adam]
    // weight-gradient stream: the dW / db GEMMs of lossgradient feed nothing but update!, so they run on their own stream beside the
    // reverse recurrences (which are chains of small launches that leave CUs idle); own split-K workspace, fork / join by events
    hipStream_t wg_stream = nullptr;
    bool wg_stream_owned = true;   // false: handed in through lrcn_set_wg_stream (not destroyed here)
    hipEvent_t wg_fork[4] = {}, wg_done = nullptr;
    hipEvent_t xc_fork = nullptr, xc_done = nullptr;  // the image-embedding GEMM of the forward pass on the weight-gradient stream (loss_impl)
    void *wg_ws = nullptr;
    void *pin = nullptr;      // pinned host staging for results larger than HIP's fast pageable-copy path (lrcn_beam_search_batch)
    size_t pin_bytes = 0;
    unsigned long long *stamps = nullptr;  // kernel-development: per-tile segment stamps (LRCN_STAMPS=1, lrcn_debug_stamps)
    int64_t stamps_n = 0;
    int *tile_ctr = nullptr;  // per-layer work queues of the capped persistent convolution grids (GemmArgs::tile_ctr)
    // input feed (lrcn_upload_crops): uint8 crops travel host -> HBM on the context's own copy stream into one of kStage staging buffers,
    // beside the running step; a VGG forward that is handed a staging buffer waits (on the device) for its upload, and the upload into a
    // staging buffer waits for the one kernel of the forward that last read it (the crops are consumed by the forward's FIRST kernel).
    // The copy stream never carries a device-side wait for a read that has not happened yet.  Measured (bench.py, host 4 steps ahead of the
    // device, which is where it runs when nothing holds it back): a hipStreamWaitEvent on an event one or two steps in the device's future
    // is a barrier packet at the head of a HARDWARE queue that the copy stream shares with compute streams (HIP maps its streams onto a few
    // hardware queues) -- kernels queued behind it stall, and the step ran 8.5 instead of 7.0 ms until the host happened to fall back.  So an
    // upload whose staging buffer is still unread BLOCKS THE CALLING THREAD (hipEventSynchronize) and then queues a copy with no dependency.
    // With kStage buffers that happens only when the host is more than kStage - 1 steps ahead of the device: a bound on the run-ahead.
    static constexpr int kStage = 3;
    hipStream_t copy_stream = nullptr;
    uint8_t *stage[kStage] = {};
    hipEvent_t up_done[kStage] = {}, rd_done[kStage] = {};
    bool stage_full[kStage] = {};   // holds crops that no forward has been issued on yet
    bool stage_read[kStage] = {};   // rd_done[j] has been recorded at least once
    int stage_next = 0;
    LrcnComm *comm = nullptr;
    hipStream_t comm_stream = nullptr;  // every collective of the communicator is issued on this ONE stream, in group order
    bool comm_stream_owned = false;     // created here (destroyed here), or handed in through lrcn_comm_set_stream
    // bucket[g] == comm_stream for every g since round 4: the groups become final in order, so one stream runs [wait, all-reduce, Adam] of
    // group after group and loses nothing, while five streams on HIP's four hardware queues meant that one of them shared a queue with the
    // VGG side stream and its Adam waited for the whole forward (dp.py streams_share_a_queue)
    hipStream_t bucket[LRCN_GRAD_GROUPS] = {};
    hipEvent_t ar_done[LRCN_GRAD_GROUPS] = {};
    hipEvent_t bucket_done[LRCN_GRAD_GROUPS] = {};
    bool bucket_pending[LRCN_GRAD_GROUPS] = {};
};

namespace lrcn_impl {

// Nothing runs beside the LSTM step: no VGG forward with capped grids on another stream (what the two-stream trainer sets up).  Its negation
// is THE test for "beside the capped convolutions"; the routes that apply there to 256..512 rows also ask bg_row_window (gemm.h).
inline bool lstm_alone(const lrcn_ctx *c) { return !(c->vgg_wg_cap >= 8 && c->vgg_loaded); }

// A pair of HIP events around one segment of a call, on the stream its work is launched on (lrcn_profile level 2; a no-op otherwise).
struct SegScope {
    lrcn_ctx *c;
    hipStream_t st;
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    SegScope(lrcn_ctx *c_, int seg, hipStream_t st_, double bytes) : c(c_), st(st_) {
        if (c->prof_level < 2) return;
        auto &sp = c->seg[seg];
        if (sp.used == sp.ev.size()) {
            std::pair<hipEvent_t, hipEvent_t> e;
            if (hipEventCreate(&e.first) != hipSuccess || hipEventCreate(&e.second) != hipSuccess) return;
            sp.ev.push_back(e);
        }
        ev = &sp.ev[sp.used++];
        sp.bytes += bytes;
        sp.n += 1;
        (void)hipEventRecord(ev->first, st);
    }
    ~SegScope() {
        if (ev) (void)hipEventRecord(ev->second, st);
    }
};

// a `void *stream` argument of the ABI: NULL means the context's stream
inline hipStream_t stream_or_ctx(lrcn_ctx *c, void *stream) { return stream ? reinterpret_cast<hipStream_t>(stream) : c->stream; }
// element counts of the context's 9 tensors (0 for the slots its model does not have)
inline void ctx_sizes(const lrcn_ctx *c, int64_t sz[9]) { lrcn_param_sizes_n(c->nl, c->E, c->H1, c->H2, c->V, sz); }
// the tensors of each gradient group, in the order of the grad_ev records in loss_impl
constexpr int kGradGroup[LRCN_GRAD_GROUPS][2] = {{7, 8}, {2, 3}, {4, 5}, {0, 1}, {6, 6}};

// C[M][N] (+)= A[M][K] * B[N][K]^T on the context's stream or (on_wg_stream) its weight-gradient stream, with its route hints (lrcn_api.hip)
int gemm(lrcn_ctx *c, int dtype, const void *A, int64_t lda, const void *B, int64_t ldb, void *C, int64_t ldc, int M, int N, int K,
         const float *bias, bool c_f32, bool beta = false, bool relu = false, bool c_is_zero = false, bool on_wg_stream = false);

#define GEMM(...)                     \
    do {                              \
        int _r = gemm(__VA_ARGS__);   \
        if (_r) return _r;            \
    } while (0)

// the text lrcn_last_error(NULL) returns: failures of the entry points that take no context (lrcn_api.hip)
void set_create_error(const char *msg);
// lrcn() on the context's single-step buffers (lrcn_api.hip): lrcn_step and the single-image beam search
int step_internal(lrcn_ctx *c, const float *const p[9], int B, const DropSpec &d2, bool h_ready = false);
// One loss / lossgradient call.  An optional pointer that is set turns its form on; the entry points of train.hip fill this by member name.
struct LossCall {
    const float *const *p = nullptr;      // the nine parameter tensors
    const float *feats = nullptr;         // B x 4096 column-major f32 (device)
    const int32_t *tokens = nullptr;      // [T][B] (device)
    int T = 0, B = 0, norm_B = 1;         // the equal-length form's scale is 1 / (norm_B (T+1)); norm_B is not used with lens
    int64_t norm_tokens = 0;              // with lens: the scale is 1 / norm_tokens
    const lrcn_dropout *drop = nullptr;
    float *const *grads = nullptr;        // NULL: forward only
    const int32_t *lens = nullptr;        // host [B]: the variable-length form (include/lrcn_varlen.h)
    const float *row_w = nullptr;         // host [B], with lens: a weight per caption (include/lrcn_weighted.h)
    const lrcn_sched *ss = nullptr;       // with lens: scheduled sampling (include/lrcn_sched.h; eps > 0: the stepwise forward)
    float smooth = 0.0f;                  // > 0, with lens: label smoothing (include/lrcn_smooth.h) -- XentCall::eps, the SMOOTH form of k_softmax_xent
    int32_t *fed_out = nullptr;           // device [T+1][B], with ss: the words that were fed
    float *logits_out = nullptr;          // device, (T+1) blocks of B x V column-major
    enum Form { PLAIN, VAR, WEIGHTED, SCHED } form = PLAIN;   // which of lens / row_w / ss the entry point requires (train.hip loss_entry checks it)
};
// loss / lossgradient on the context's buffers (train.hip)
int loss_impl(lrcn_ctx *c, const LossCall &q);
// waits for the context's stream; the last loss call's mean loss into *out (NULL: only the out-of-range-token check) (train.hip)
int fetch_loss(lrcn_ctx *c, double *out);
// Which shadows a prepare_weights call needs on top of the forward ones.  cat, cat_perm and dec_tables belong to the batched decode.
struct ShadowNeed {
    bool bwd = false;         // the transposed copies of the backward pass
    bool cat = false;         // W1cat / W2cat: [x | h] side by side, one gate GEMM per LSTM
    bool gi = false;          // the recurrent weights with (unit, gate)-interleaved rows (cell-epilogue routes); sticky under the fused update
    bool cat_perm = false;    // with cat: their rows interleaved likewise
    bool dec_tables = false;  // gi and dec_W2c (W2 without its x_cnn columns, rows interleaved): a decode call, not sticky
};
// f32 column-major params -> K-contiguous shadows in T (update.hip; see DESIGN.md "shadow weights")
int prepare_weights(lrcn_ctx *c, const float *const p[9], const ShadowNeed &need = ShadowNeed{});
// the second shadow set of LRCN_OPT_FUSED_UPDATE, allocated once (update.hip): lrcn_set_option makes it outside any step
int ensure_alt_shadows(lrcn_ctx *c);
// update! of all nine tensors / of one gradient group on `stream` (update.hip): lrcn_adam_update[_group] and, `clipped`, their clipped
// namesakes, argument checks included
int adam_update(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step, float lr, float b1,
                float b2, float eps, bool clipped);
int adam_update_group(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group, int step,
                      float lr, float b1, float b2, float eps, void *stream, bool clipped);
// the VGG-16 forward of N images into featsRM (vgg.hip): lrcn_train_step_dp and the image entry points
int vgg_body(lrcn_ctx *c, int N, const void *src, bool src_u8, const float *mean, bool calibrate = false);
int vgg_check(lrcn_ctx *c, int N);

}  // namespace lrcn_impl
