/* lrcn_smooth.h -- label smoothing (Szegedy et al. 2016) in the cross-entropy stage of caption training: loss, gradient and training step
 * whose target distribution is softened inside the softmax-NLL kernels, and that stage alone on a caller's own logits, beside the C ABI of
 * include/lrcn.h (LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry
 * points. */
#ifndef LRCN_SMOOTH_H
#define LRCN_SMOOTH_H

#include "lrcn_sched.h"

#ifdef __cplusplus
extern "C" {
#endif

/* eps = smooth, 0 <= eps <= 1.  An active row (a step s <= lens[b] of a caption whose weight is not 0) with logits z over V columns, gold
 * target t and row scale sc = row_w[b] / norm_tokens (the weight 1 without row_w) is scored against q = (1 - eps) onehot(t) + eps / V,
 * uniform over ALL V columns (torch.nn.functional.cross_entropy(label_smoothing=eps)):
 *
 *   m  = max_v z_v                     se = sum_v exp(z_v - m)
 *   ll = (z_t - m) - log se            the plain log-likelihood term
 *   u  = (1 / V) sum_v (z_v - m) - log se      the mean log-probability
 *   row term   = row_w[b] ((1 - eps) ll + eps u)          summed in double; loss = -(sum of the terms) / norm_tokens
 *   d(logits)_v = (exp(z_v - m) / se - (1 - eps) [v == t] - eps / V) sc     f32; rounded once where it is stored in a bf16 context
 *
 * An inactive row behaves as in lrcn_weighted.h: term 0, an all-zero d(logits) row, its logits never read.  The sum of (z_v - m) rides in
 * the pass that forms the exponentials; everything after the softmax-NLL launch is the other calls' and linear in d(logits).
 *
 * The batch is the padded batch of lrcn_sched.h: lens HOST int32 [B] is required (an equal-length caller passes lens[b] = T), row_w HOST
 * float [B] may be NULL.  ss may be NULL or have eps 0 (the time-batched route); ss->eps > 0 takes the stepwise forward of scheduled
 * sampling -- the draw reads logits, so smoothing does not touch it, and fed_out (device int32 [T+1][B] or NULL) receives the same words
 * as lrcn_loss_grad_sched's.
 *
 * smooth == 0 runs the kernels of the other headers: the call returns the bits of lrcn_{loss, loss_grad, train_step}_sched with the same
 * arguments (of _w / _var with a NULL ss).
 *
 * *loss_host (may be NULL) is the SMOOTHED loss, and so is lrcn_last_loss; lrcn_smooth_stats has the plain one.
 *
 * LRCN_EINVAL before any GPU work: a NaN smooth or one outside [0, 1], and everything lrcn_loss_grad_sched rejects but a NULL ss. */
int lrcn_loss_smooth(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                     const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss, int32_t *fed_out,
                     float smooth, double *loss_host);
int lrcn_loss_grad_smooth(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                          const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss,
                          int32_t *fed_out, float smooth, float *const grads[9], double *loss_host);
/* lrcn_loss_grad_smooth followed by the update; max_norm as in lrcn_train_step_sched. */
int lrcn_train_step_smooth(lrcn_ctx *ctx, float *const params[9], float *const grads[9], float *const mom[9], float *const var[9],
                           const float *feats, const int32_t *tokens, const int32_t *lens, const float *row_w, int T, int B,
                           int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss, float smooth, int step, float lr, float beta1,
                           float beta2, float eps_adam, float max_norm, double *loss_host);
/* Of the most recent *_smooth call, as long as no other loss call has followed it: *smoothed = its loss, *nll = the same sum with eps = 0
 * (-(sum of row_w[b] ll) / norm_tokens, which the kernels add up in a second accumulator), so a training loop can still log the plain
 * negative log-likelihood.  After a call with smooth == 0 the two are equal.  Waits for the context's stream.  Either pointer may be NULL.
 * LRCN_ESTATE when the context has made no *_smooth call. */
int lrcn_smooth_stats(lrcn_ctx *ctx, double *nll, double *smoothed);

/* The cross-entropy stage alone, on the caller's own logits (all pointers DEVICE memory): M rows of V f32, ld apart.  Row m belongs to
 * caption m % B and reads row_w[m % B] (row_w f32 [B], or NULL: every weight 1); tgt int32 [M], and a target outside [0, V) -- a negative
 * one is the padded batch's marker -- or a weight 0 makes the row inactive.  An active row's scale is sc = scale * row_w[m % B].
 *
 *   dlog      [M] rows ld_d apart of f32 (out_dtype LRCN_F32) or bf16 (LRCN_BF16), or NULL: d(logits) as above
 *   terms     double [M] or NULL: the rows' smoothed terms row_w ((1 - eps) ll + eps u)
 *   ll_terms  double [M] or NULL: the rows' plain terms row_w ll
 *
 * Inactive rows get term 0 and an all-zero dlog row.  Nothing is summed and nothing is copied to the host; the launches are on the
 * context's stream.  smooth == 0 runs the kernels of lrcn_loss_grad_var (row_w NULL) or lrcn_loss_grad_w, and terms equals ll_terms.
 * The route is the training step's: rows held in registers up to V = 16384 when logits and dlog are 16-byte aligned and ld % 4 == 0,
 * else a streaming kernel.
 *
 * LRCN_EINVAL before any GPU work: a NULL logits or tgt, M, B or V < 1, ld < V, dlog with ld_d < V, an out_dtype that is neither,
 * a NaN or infinite scale, a NaN smooth or one outside [0, 1]. */
int lrcn_xent_logits(lrcn_ctx *ctx, const float *logits, int64_t ld, const int32_t *tgt, const float *row_w, int M, int B, int V,
                     float scale, float smooth, int out_dtype, void *dlog, int64_t ld_d, double *terms, double *ll_terms);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_SMOOTH_H */
