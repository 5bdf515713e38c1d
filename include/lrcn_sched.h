/* lrcn_sched.h -- scheduled sampling (Bengio et al. 2015) in the cross-entropy stage of caption training: loss, gradient and training
 * step in which a row's next input word is, with probability eps, drawn on the device from the row's own logits of the step before, beside
 * the C ABI of include/lrcn.h (LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these
 * entry points. */
#ifndef LRCN_SCHED_H
#define LRCN_SCHED_H

#include "lrcn_weighted.h"

#ifdef __cplusplus
extern "C" {
#endif

/* eps: the probability that an eligible input is the model's own word (0 <= eps <= 1); temperature: of the draw (0 = argmax); seed: the
 * Philox key of coins and noise; row0: the index of this call's row 0 in the GLOBAL batch (0 on one device; a data-parallel rank's first
 * row), so that coins and noise depend on (seed, global row, step) alone and not on how a batch is cut over ranks. */
typedef struct {
    float eps;
    float temperature;
    uint64_t seed;
    int64_t row0;
} lrcn_sched;

/* The batch is the padded batch of lrcn_varlen.h (tokens device [T][B]; lens HOST int32 [B], required -- an equal-length caller passes
 * lens[b] = T); row_w is as in lrcn_weighted.h and may be NULL: every weight 1.  Targets are always the gold words.  The INPUT of row b:
 *
 *   s = 0                bos
 *   1 <= s <= lens[b]    the gold word tokens[s-1][b], unless the row's coin of step s fires: then a word drawn from the row's own logits
 *                        of step s-1, as the training forward (dropout on) computed them
 *   s > lens[b]          eos, as in lrcn_loss_grad_var; no coin is taken, nothing is drawn
 *
 * Coin of (s, b).  x = word 0 of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (0xFFFFFFFF, s, 0xFFFFFFFF,
 * (uint32)(row0 + b)); u = ((x >> 9) + 0.5) * 2^-23 in float32; the coin fires iff u < eps.  (Counter word 0 of a noise call is a column
 * index / 4: it never is 0xFFFFFFFF.)  The smallest u is 2^-24, so no coin fires below that eps, and every coin fires at eps = 1.
 *
 * Draw of (s, b).  The draw of lrcn_sample.h with top_k = 0: tok = argmax_j (z_j / temperature + g_j) over the columns j with
 * z_j >= max z - 20 * temperature, the lowest column winning a tie; z = the f32 logits row of step s-1, g_j the Gumbel noise of Philox
 * counter (j >> 2, s, 0, (uint32)(row0 + b)), word j & 3.  temperature == 0 is the argmax of z.
 *
 * Gradient.  The fed word is a constant: nothing flows through the draw.  Loss and gradients are those of lrcn_loss_grad_var /
 * lrcn_loss_grad_w with the inputs replaced by the fed words (the embedding gradient lands on the fed words' rows).
 *
 * eps == 0: the call takes the time-batched route and returns the bits of lrcn_loss_grad_var (row_w NULL) or lrcn_loss_grad_w.
 * 0 < eps <= 1: the forward runs step by step -- step s+1's input is decided and gathered by one kernel after step s's logits -- into
 * the same activation buffers; softmax-NLL, the backward pass, the gradient-group events, the sparse embedding-row export and the
 * clipped update are the time-batched route's.
 *
 * Repeatability.  On a context with LRCN_OPT_DETERMINISTIC two identical calls return identical fed words, loss and gradients.  Without
 * that option nothing is promised about the draws: the forward's split-K sums may differ in their last bits.
 *
 * fed_out    device int32 [T+1][B] or NULL: the words that were fed.
 * logits_out device f32 in the layout of lrcn_forward_logits ((T+1) blocks of B x V column-major) or NULL: the logits the draws were
 *            made from.
 *
 * LRCN_EINVAL before any GPU work: ss NULL, eps NaN or outside [0, 1], temperature NaN, negative or infinite, row0 < 0 or
 * row0 + B > 2^32, a NULL lens, and everything lrcn_loss_grad_w rejects (a NULL row_w is allowed here). */
int lrcn_loss_sched(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                    const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss,
                    int32_t *fed_out, float *logits_out, double *loss_host);
int lrcn_loss_grad_sched(lrcn_ctx *ctx, const float *const params[9], const float *feats, const int32_t *tokens, const int32_t *lens,
                         const float *row_w, int T, int B, int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss,
                         float *const grads[9], int32_t *fed_out, float *logits_out, double *loss_host);
/* lrcn_loss_grad_sched followed by the update; max_norm as in lrcn_train_step_w (<= 0: unclipped, > 0: the device clipping of
 * include/lrcn_clip.h). */
int lrcn_train_step_sched(lrcn_ctx *ctx, float *const params[9], float *const grads[9], float *const mom[9], float *const var[9],
                          const float *feats, const int32_t *tokens, const int32_t *lens, const float *row_w, int T, int B,
                          int64_t norm_tokens, const lrcn_dropout *drop, const lrcn_sched *ss, int step, float lr, float beta1, float beta2,
                          float eps_adam, float max_norm, double *loss_host);
/* The most recent scheduled-sampling call's counts, from two integer counters on the device: eligible = sum of lens[b] (the coins
 * taken), drawn = the coins that fired.  Waits for the context's stream.  Either pointer may be NULL. */
int lrcn_sched_stats(lrcn_ctx *ctx, int64_t *eligible, int64_t *drawn);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_SCHED_H */
