/* lrcn_clip.h -- clipping of the GLOBAL gradient norm on the device, beside the C ABI of include/lrcn.h (which it includes;
 * LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points.
 *
 * The reference declares --gclip and never applies it (its clipping block is commented out).  Here the norm is taken on the device and
 * the Adam kernels pick the scale factor up from device memory, so no call but lrcn_clip_stats waits for the GPU.
 *
 * The context owns a control block: up to LRCN_CLIP_SLOTS sums of squares (doubles), and norm / scale / skip / counters.
 *
 *   slot[k]  = sum_i (double)g_k[i]^2         lrcn_grad_sumsq / lrcn_grad_sumsq_model: a fixed summation order, no atomics -- the value
 *                                             depends on the data and on n alone, not on the stream, the timing or the pointer's alignment
 *   norm     = sqrt(slot[0] + ... + slot[n_slots - 1])          added in slot order, in double          (lrcn_clip_set)
 *   skip     = !isfinite(norm)
 *   scale    = (!skip && norm > (double)max_norm) ? (float)((double)max_norm / norm) : 1.0f
 *
 * A clipped update is the plain update on g[i] * scale (one float multiply per element, then the unchanged Adam arithmetic).  The gradient
 * buffers are NOT scaled in place: callers keep the unclipped gradient, the scale is in lrcn_clip_stats.  With skip set (an inf or NaN in
 * the gradient) the update writes none of w, m, v: the step is dropped instead of poisoning the moments.  Under LRCN_OPT_FUSED_UPDATE a
 * skipped update still writes the next step's shadow weights (from the unchanged parameters) and the shadow sets swap as after any update.
 * The caller's `step` advances whether or not the update was skipped: Adam's bias correction counts calls, not applied updates.
 *
 * LRCN_EINVAL before any GPU work: NULL pointers, a slot or group out of range, n < 0, n_slots outside [1, LRCN_CLIP_SLOTS], a NaN max_norm (lrcn_clip_set: any max_norm that is not > 0),
 * and everything the plain namesake of a call rejects. */
#ifndef LRCN_CLIP_H
#define LRCN_CLIP_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LRCN_CLIP_SLOTS 9

typedef struct lrcn_clip_stats_t {
    double last_norm;     /* of the last lrcn_clip_set */
    float last_scale;     /* 1 when that step was not clipped (or was skipped) */
    int32_t last_skipped; /* 1: the last norm was not finite, the update that read it wrote nothing */
    int64_t steps;        /* lrcn_clip_set calls since the context was created */
    int64_t clipped;      /* ... of which scale < 1 was applied */
    int64_t skipped;      /* ... of which the norm was not finite */
} lrcn_clip_stats_t;

/* slot[slot] = sum of squares of the device run g[0..n) (n = 0 writes 0), on `stream` (NULL: the context's stream). */
int lrcn_grad_sumsq(lrcn_ctx *ctx, const float *g, int64_t n, int slot, void *stream);
/* Tensor k's sum of squares into slot k, for the tensors of gradient group `group` (see lrcn_grad_group_wait), or all nine with
 * group = -1.  The empty tensors of an LRCN-1f model write 0. */
int lrcn_grad_sumsq_model(lrcn_ctx *ctx, const float *const grads[9], int group, void *stream);
/* Device address of slot[0..LRCN_CLIP_SLOTS): a sharded job all-reduces its ranks' partial sums in place before lrcn_clip_set. */
int lrcn_clip_slots(lrcn_ctx *ctx, double **dev_ptr);
/* norm, skip and scale from the first n_slots slots, as defined above; bumps the counters.  max_norm must be > 0. */
int lrcn_clip_set(lrcn_ctx *ctx, int n_slots, float max_norm, void *stream);

/* lrcn_adam_update / _group / _flat reading scale and skip from the control block: same arguments, same fused / unfused routing, same
 * shadow bookkeeping as the plain calls. */
int lrcn_adam_update_clipped(lrcn_ctx *ctx, float *const params[9], const float *const grads[9], float *const mom[9], float *const var[9],
                             int step, float lr, float beta1, float beta2, float eps);
int lrcn_adam_update_group_clipped(lrcn_ctx *ctx, float *const params[9], const float *const grads[9], float *const mom[9],
                                   float *const var[9], int group, int step, float lr, float beta1, float beta2, float eps, void *stream);
int lrcn_adam_update_flat_clipped(lrcn_ctx *ctx, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float beta1,
                                  float beta2, float eps, void *stream);

/* lrcn_train_step / lrcn_train_step_var with the global norm clipped to max_norm: loss-gradient, the nine sums of squares, lrcn_clip_set(9)
 * and the clipped update, all on the context's stream, no host wait.  max_norm <= 0: exactly the plain call (the control block is not
 * touched). */
int lrcn_train_step_clip(lrcn_ctx *ctx, float *const params[9], float *const grads[9], float *const mom[9], float *const var[9],
                         const float *feats, const int32_t *tokens, int T, int B, int norm_B, const lrcn_dropout *drop, int step, float lr,
                         float beta1, float beta2, float eps, float max_norm, double *loss_host);
int lrcn_train_step_var_clip(lrcn_ctx *ctx, float *const params[9], float *const grads[9], float *const mom[9], float *const var[9],
                             const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B, int64_t norm_tokens,
                             const lrcn_dropout *drop, int step, float lr, float beta1, float beta2, float eps, float max_norm,
                             double *loss_host);

/* Waits for the context's stream and copies the control block's results out: the only call here that blocks.  Work queued on OTHER
 * streams (the `stream` arguments above) must have been joined into the context's stream by the caller. */
int lrcn_clip_stats(lrcn_ctx *ctx, lrcn_clip_stats_t *host_out);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_CLIP_H */
