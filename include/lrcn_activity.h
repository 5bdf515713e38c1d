/* lrcn_activity.h -- LRCN activity recognition (paper section 4): one LSTM layer over per-frame CNN features, a softmax over C action
 * classes at every time step, and a clip's prediction the mean of its per-step distributions.  Beside the C ABI of include/lrcn.h (which
 * it includes; lrcn.h, its exports and LRCN_ABI_VERSION are unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not
 * implement these entry points.
 *
 * Model.  params[4] are device f32 arrays, column-major, in the convention of lrcn_lstm:
 *   [0] W    (F+H) x 4H   gate column blocks [forget | in | out | change]; rows 0..F-1 read the frame feature, rows F..F+H-1 the hidden state
 *   [1] b    1 x 4H
 *   [2] Wout H x C
 *   [3] bout 1 x C
 * Clip b of a call has T frames, of which the first len_b are real (1 <= len_b <= T).  h_{-1} = c_{-1} = 0 and
 *   (h_t, c_t) = lstm(W, b, x_{t,b}, h_{t-1}, c_{t-1})        (exactly lrcn_lstm with X = F on the same W / b)
 *   z_{t,b} = h_t Wout + bout,   p_{t,b} = softmax(z_{t,b})
 *   loss = -(1 / sum_b len_b) * sum_b sum_{t < len_b} log p_{t,b}[label_b]
 *   clip_probs[:, b] = (1 / len_b) * sum_{t < len_b} p_{t,b}
 * Steps t >= len_b are computed (the recurrence is causal, so they never reach a step t < len_b) and then ignored: no loss, no gradient,
 * no share of the average.
 *
 * Features.  feats is (B*T) x F column-major f32 on the device, row n = b*T + t (clip-major): what lrcn_vgg_forward_u8 writes for the B*T
 * frames of B clips in order.  It is read by pointer; any lrcn_ctx on the same device may have made it.  No gradient flows to it.
 *
 * Arithmetic.  dtype LRCN_F32: every contraction in exact f32.  LRCN_BF16: the operands of every contraction are rounded to bf16 and
 * accumulated in f32 -- the frame features, W, Wout and h in the forward pass.  The cell update is f32 (c is f32); the activated gates
 * f, i, o, g are stored as bf16, and the backward pass reads those copies; h_t is rounded to bf16 where it is stored (the next step and
 * the head read that copy).  Gx = X W[0:F] + b and the recurrent pre-activations are f32.  Logits, softmax, clip averages and the head's dlogits
 * (softmax - onehot) / sum len are computed in f32; the loss is summed in double.  Backward: dlogits are rounded to bf16 once, and that
 * copy is the operand of dWout, of dh = dlogits Wout' and of the column sum dbout; the gate gradients dZ are rounded to bf16 where they are
 * stored (operand of dW, of the recurrent dh and of the column sum db); dh, dc are f32.  This is the caption path's convention.
 *
 * Route.  Gx for all T*B frames is one GEMM (time-major rows t*B + b).  The recurrence then contracts h only: in bf16 with the fused
 * step kernels of the caption path (lstm_fused.hip) where they apply (B <= 128 by default, as the caption path; LRCN_LSTM_FUSED=0 turns
 * them off, read per call), else one GEMM + one cell kernel per step.  The head (log-softmax, the masked NLL term, dlogits, the clip
 * average) runs one workgroup per clip over its T rows in order; the per-clip loss terms are summed in clip order.  With deterministic = 1
 * every GEMM takes its ordered form and the bias column sums their single-slab form: two identical calls give bit-identical loss,
 * gradients and probabilities.  Without it the loss and the probabilities are still reproducible (no float atomics in the head).
 *
 * Every call is queued on the handle's stream (lrcn_act_set_stream; default the null stream); the call returns after queueing unless it
 * hands back a host value (loss_host != NULL, clip_probs / frame_probs are device arrays).  Bad arguments return LRCN_EINVAL before any
 * GPU work: T outside [1, max_T], B outside [1, max_B], a label outside [0, C), a length outside [1, T], a NULL pointer. */
#ifndef LRCN_ACTIVITY_H
#define LRCN_ACTIVITY_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrcn_act lrcn_act;

typedef struct {
    int device;         /* HIP device ordinal */
    int F, H, C;        /* feature width, hidden units, classes (all >= 1; C <= 4096) */
    int max_B, max_T;   /* largest clips per call and steps per clip (max_B * max_T < 2^31 / max(F, 4H)) */
    int dtype;          /* LRCN_F32 | LRCN_BF16 */
    int deterministic;  /* 1: every floating-point sum in a fixed order (bit-identical repeats of lrcn_act_loss_grad) */
} lrcn_act_config;

/* The handle owns its scratch, sized for max_B clips of max_T frames, and nothing else (no caption model, no VGG). */
int lrcn_act_create(const lrcn_act_config *cfg, lrcn_act **out);
void lrcn_act_destroy(lrcn_act *act);
const char *lrcn_act_last_error(const lrcn_act *act);   /* act may be NULL: the last creation error */
int lrcn_act_set_stream(lrcn_act *act, void *hip_stream); /* hipStream_t; NULL = null stream */

/* Element counts of W, b, Wout, bout. */
int lrcn_act_param_sizes(int F, int H, int C, int64_t sizes[4]);
/* xavier-uniform +-sqrt(2 / (rows + cols)) for W and Wout, zero biases, forget-gate bias 1: the rule and counter-hash generator of
 * lrcn_init_weights, keyed by (seed, tensor 0 for W / 7 for Wout -- the caption model's W1 and Wout slots, index). */
int lrcn_act_init_weights(lrcn_act *act, float *const params[4], uint64_t seed);

/* labels [B] (0-based class ids) and lens [B] (NULL: every clip has T frames) are HOST int32 arrays.  grads[4] (device, overwritten) may
 * be NULL: the loss only.  loss_host (may be NULL) receives the loss (the call then synchronises). */
int lrcn_act_loss_grad(lrcn_act *act, const float *const params[4], const float *feats, const int32_t *labels, const int32_t *lens, int T,
                       int B, float *const grads[4], double *loss_host);

/* clip_probs: device f32 C x B column-major (column b = clip b).  frame_probs (may be NULL): device f32 C x (B*T) column-major, column
 * b*T + t = p_{t,b} for t < len_b and zeros for t >= len_b. */
int lrcn_act_predict(lrcn_act *act, const float *const params[4], const float *feats, const int32_t *lens, int T, int B, float *clip_probs,
                     float *frame_probs);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_ACTIVITY_H */
