/* lrcn_weighted.h -- caption loss, gradient and training step in which every caption row carries a real weight of its own, beside the C ABI
 * of include/lrcn.h (LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry
 * points. */
#ifndef LRCN_WEIGHTED_H
#define LRCN_WEIGHTED_H

#include "lrcn_varlen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The padded batch of lrcn_varlen.h (tokens device [T][B]; lens HOST int32 [B], 0 <= lens[b] <= T) with row_w: HOST float [B], read
 * before the call returns.  A weight may be positive, negative or zero:
 *
 *   loss = -(1 / norm_tokens) * sum_b row_w[b] * sum_{s <= lens[b]} log p_{s,b}[y_{s,b}]
 *
 * This is the policy-gradient loss of self-critical sequence training (row_w[b] = reward of sample b minus its baseline), and it serves
 * importance weights and "this row does not count" without re-packing a batch.  norm_tokens is the caller's: lrcn_varlen.h's rule (the
 * GLOBAL batch's sum of lens[b] + 1 under data parallelism) keeps a step's scale comparable with a cross-entropy step on the same
 * captions; zero-weight rows may be counted or not.
 *
 * How.  Only the softmax-NLL launch differs from lrcn_loss_grad_var.  Row m = s B + b of the (T + 1) B logits rows reads row_w[b]:
 *   row_w[b] == 0   the row is inactive, exactly as a step past its caption's end: no loss term, an all-zero d(logits) row, its
 *                   logits never read (one zero-fill instead of a softmax).  Loss and gradients then do not depend on that
 *                   row's tokens, as they do not depend on padding
 *   otherwise       d(logits) = (p - onehot) * (f32)(scale * row_w[b]), the term row_w[b] * log p in double
 * Everything after that launch is linear in d(logits).  With every weight 1.0f the three calls return the bits of lrcn_loss_var /
 * lrcn_loss_grad_var / lrcn_train_step_var(_clip) on a deterministic context.
 *
 * Dropout, both layer counts, both LSTM types, the gradient-group events, lrcn_last_loss and LRCN_OPT_DETERMINISTIC behave as in
 * lrcn_loss_grad_var.  lens is required: an equal-length caller passes lens[b] = T.
 *
 * LRCN_EINVAL before any GPU work: a NULL lens, a NULL row_w, a NaN or infinite weight, and everything lrcn_loss_grad_var rejects. */
int lrcn_loss_w(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, double *loss_host);
int lrcn_loss_grad_w(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                     const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, float *const grads[9],
                     double *loss_host);
/* lrcn_loss_grad_w followed by the update.  max_norm <= 0: the unclipped update of lrcn_train_step_var.  max_norm > 0: the device
 * clipping of lrcn_train_step_var_clip (include/lrcn_clip.h) -- the nine sums of squares, lrcn_clip_set and the clipped Adam, no host
 * wait. */
int lrcn_train_step_w(lrcn_ctx *ctx, float *const params[9], float *const grads[9], float *const mom[9], float *const var[9],
                      const float *feats, const int32_t *tokens, const int32_t *lens, const float *row_w, int T, int B, int64_t norm_tokens,
                      const lrcn_dropout *drop, int step, float lr, float beta1, float beta2, float eps, float max_norm, double *loss_host);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_WEIGHTED_H */
