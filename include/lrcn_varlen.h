/* lrcn_varlen.h -- caption loss, gradient and training step over batches whose captions differ in length, beside the C ABI of include/lrcn.h
 * (which it includes; LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry
 * points. */
#ifndef LRCN_VARLEN_H
#define LRCN_VARLEN_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The padded (masked) batch.  tokens: device [T][B], 0-based, as lrcn_loss takes them; lens: HOST int32 [B], 0 <= lens[b] <= T (read before
 * the call returns).  Row b has lens[b] + 1 loss terms: inputs bos, tok(0..len-1), targets tok(0..len-1), eos.  tokens[t][b] at
 * t >= lens[b] is never read (any value may stand there), so padding cannot raise the out-of-range flag; an id outside [0, V) at an
 * active position still does, as in lrcn_loss.
 *
 *   loss = -(1 / norm_tokens) * sum_b sum_{s <= lens[b]} log p_{s,b}[y_{s,b}]
 *
 * norm_tokens: on one device sum_b (lens[b] + 1); under data parallelism the same sum over the GLOBAL batch, on every rank -- norm_B's role:
 * the ranks' gradients then sum to the single-device gradient.  With lens[b] = T for every row and norm_tokens = norm_B (T + 1) the three
 * calls launch what lrcn_loss / lrcn_loss_grad / lrcn_train_step launch with the same scale, and a deterministic context returns the
 * same bits.
 *
 * Dropout (pdrop + seed or explicit masks, over all T + 1 steps), both layer counts and both LSTM types behave as in lrcn_loss_grad.  The
 * gradient-group events of lrcn_grad_group_wait are recorded as by lrcn_loss_grad, and lrcn_last_loss works after these calls.
 *
 * How.  The LSTM is causal: a step past a caption's end cannot reach an earlier one, so only the loss terms need a mask.  The token
 * builder gives a step s > lens[b] the input eos and marks it inactive; the softmax-NLL kernel gives an inactive row no loss term
 * and an all-zero d(logits) row without reading its logits.  Everything between runs exactly as for equal lengths ("compute and ignore").
 * In the backward pass an inactive step has a zero d(logits) row and no later active step of its row, so its dh, dc, d(gates) and dx
 * are exact zeros: they add exact zeros to every weight and bias gradient and to eos's row of the embedding gradient.  Hence loss and
 * gradients do not depend on what the padding holds.
 *
 * LRCN_EINVAL before any GPU work: a NULL lens, a length outside [0, T], norm_tokens < 1, and everything lrcn_loss_grad rejects. */
int lrcn_loss_var(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B,
                  int64_t norm_tokens, const lrcn_dropout *drop, double *loss_host);
int lrcn_loss_grad_var(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B,
                       int64_t norm_tokens, const lrcn_dropout *drop, float *const grads[9], double *loss_host);
/* lrcn_loss_grad_var followed by lrcn_adam_update, as lrcn_train_step. */
int lrcn_train_step_var(lrcn_ctx *ctx, float *const params[9], float *const grads[9], float *const mom[9], float *const var[9],
                        const float *feats, const int32_t *tokens, const int32_t *lens, int T, int B, int64_t norm_tokens,
                        const lrcn_dropout *drop, int step, float lr, float beta1, float beta2, float eps, double *loss_host);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_VARLEN_H */
