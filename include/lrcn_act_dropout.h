/* lrcn_act_dropout.h -- seeded dropout for activity training: on the frame feature that enters the LSTM and on the LSTM output before
 * the classifier (the paper's activity networks use 0.9 and 0.5).  Beside include/lrcn_activity.h (which it includes; that header, its
 * exports and LRCN_ABI_VERSION are unchanged).  Implemented by liblrcn_hip.so only.
 *
 * Model.  With multipliers m_in(t,b,f) and m_out(t,b,j) in {0, 1 / (1 - p)}:
 *   x'_{t,b} = x_{t,b} .* m_in(t,b,:)
 *   (h_t, c_t) = lstm(W, b, x'_{t,b}, h_{t-1}, c_{t-1})        (the recurrent h is NOT masked)
 *   z_{t,b} = (h_t .* m_out(t,b,:)) Wout + bout
 * and the loss and the gradients are those of this masked forward pass, otherwise exactly as lrcn_act_loss_grad: lengths, the normaliser
 * 1 / sum_b len_b, grads == NULL (the loss only) and loss_host == NULL behave the same.  drop == NULL is the plain call, and a call whose
 * two sides are both the identity (p == 0 and no mask) launches what lrcn_act_loss_grad launches: bit-identical results.
 * lrcn_act_predict never drops.
 *
 * Masks.  The generator is the caption path's (csrc/kernel_util.h drop_mult): element (t, b, j) of a T x [B x ncols] tensor has the counter
 * (t*B + b)*ncols + j and is kept iff hash_uniform(seed, which, counter) > p, with the multiplier 1.0f / (1.0f - p), all in float32;
 * which = 1 and ncols = F for the frames, which = 2 and ncols = H for the LSTM output.  So a clip's mask depends on its position b in the
 * batch and on B: the same clip at another position, or in a batch of another size, draws another mask under the same seed.
 * An explicit mask (device f32) replaces (p, seed) on its side: element (t, b, j) at (t*ncols + j)*B + b, T column-major blocks of B x ncols
 * (DropSpec::mask's layout), any multipliers.  Masks of steps t >= len_b are evaluated and have no effect on the loss or a gradient.
 *
 * Arithmetic (beside the rounding list of lrcn_activity.h).  LRCN_F32: everything f32.  LRCN_BF16, forward: X = bf16(feat_f32 * m_in), one
 * rounding, after the product; the recurrence stores h_t as bf16 as before (the next step reads that unmasked copy); the head's operand is a
 * second copy Hd = bf16(f32(h_bf16) * m_out).  Backward: dWout contracts Hd; dh = (dlogits Wout') * m_out in f32; dW[0:F] contracts the
 * masked X (X and its transpose are written from the same masked tile).
 *
 * With deterministic = 1 two identical calls give bit-identical loss and gradients, and a call with (p, seed) equals the call with the same
 * multipliers given as explicit masks bit for bit (the masks are generated, never summed: no atomics).
 *
 * Errors.  LRCN_EINVAL before any GPU work, grads untouched: p_in or p_out NaN, < 0 or >= 1, and every argument error of
 * lrcn_act_loss_grad. */
#ifndef LRCN_ACT_DROPOUT_H
#define LRCN_ACT_DROPOUT_H

#include "lrcn_activity.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float p_in, p_out;               /* drop probabilities, each in [0, 1); 0 = identity */
    uint64_t seed;                   /* counter-hash key */
    const float *mask_in, *mask_out; /* device f32 multipliers or NULL; a mask given replaces (p, seed) on its side */
} lrcn_act_dropout;

int lrcn_act_loss_grad_drop(lrcn_act *act, const float *const params[4], const float *feats, const int32_t *labels, const int32_t *lens,
                            int T, int B, const lrcn_act_dropout *drop, float *const grads[4], double *loss_host);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_ACT_DROPOUT_H */
