// train_dp.hip -- data parallelism of the caption model's training step: the RCCL communicator of a context (comm.h), the per-group
// [gradient ready -> all-reduce -> Adam] pipeline on the communicator's stream, the sparse exchange of the embedding gradient, and
// lrcn_train_step_dp, one rank's whole step (VGG forward, lossgradient, exchange, update) in one call.
#include "ctx.h"

using namespace lrcn_impl;

namespace {

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

extern "C" {

int lrcn_comm_unique_id(void *id_out) {
    if (!id_out) return LRCN_EINVAL;
    char err[256] = "";
    if (comm_unique_id(id_out, err, sizeof(err))) {
        set_create_error(err);
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
    hipStream_t st = stream_or_ctx(c, stream);
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
    LossCall q{};
    q.p = p; q.feats = feats; q.tokens = tokens; q.T = T; q.B = B; q.norm_B = norm_B; q.drop = drop; q.grads = g;
    r = loss_impl(c, q);
    if (r) return r;
    if (!c->comm || (comm_world(c->comm) == 1 && !dp_force_pipeline())) {  // one rank: nothing to hide the update behind -- one Adam launch
        r = adam_update(c, p, g, m, v, step, lr, b1, b2, eps, false);
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
        r = adam_update_group(c, p, g, m, v, grp, step, lr, b1, b2, eps, c->bucket[grp], false);
        if (r) return r;
    }
    r = join_buckets(c);  // the next step's shadow-weight pass reads the updated parameters
    if (r) return r;
    return loss_host ? fetch_loss(c, loss_host) : LRCN_OK;
}

}  // extern "C"
