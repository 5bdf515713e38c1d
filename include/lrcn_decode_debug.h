/* lrcn_decode_debug.h -- the batched decode step (decode_begin / decode_step of csrc/decode.hip) with caller-given input tokens and parent
 * rows, its states and logits copied out after every step: the test entry of the three step forms decode_route chooses between, beside the
 * C ABI of include/lrcn.h (which it includes; LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not
 * implement this entry point. */
#ifndef LRCN_DECODE_DEBUG_H
#define LRCN_DECODE_DEBUG_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrcn_decode_debug {
    const float *const *params;   /* the 9 device parameter arrays, as lrcn_beam_search_batch takes them */
    const float *feats;           /* device, N x 4096 column-major f32 */
    int N, per_image, steps;      /* R = N * per_image rows; row r belongs to image r / per_image */
    const int32_t *tokens;        /* HOST [steps][R]: the input token of row r at step s */
    const int32_t *parents;       /* HOST [steps][R]: row r at step s continues the states row parents[s][r] had after step s-1; step 0's row is not read */
    void *h1, *h2;                /* device [steps][R][H1] / [steps][R][H2] in the context's LSTM element type, copied as stored (nothing converted) */
    float *c1, *c2;               /* device f32 [steps][R][H1] / [H2] */
    float *logits;                /* device f32 [steps][R][V] (dense: the entry strips ldV) */
    int route;                    /* out: 0 plain, 1 epi, 2 tables -- what decode_route chose */
} lrcn_decode_debug;

/* `steps` steps of the batched decode on the route decode_route picks for R rows (the LRCN_DECODE_* knobs are honoured as the generation
 * entries honour them), the logits written as f32 (no softmax / top-K tail).  Step s feeds tokens[s] and, from the second step, continues
 * the states of parents[s]: on the tables and cell-epilogue routes the step reads them through the parent index, on the plain route the
 * states are gathered before the step (what the beam does after the previous one).  After every step c1, c2, that step's h1, h2 and the
 * logits are copied to the caller's arrays.  LRCN-1f (n_layers == 1): h2 and c2 may be NULL, the logits come from h1.
 * LRCN_EINVAL before any launch, with the outputs (route included) untouched, when an argument is NULL, N, per_image or steps < 1,
 * N * per_image > max_B, a token is outside [0, V) or a parent of a step >= 1 outside [0, R).  Allocates nothing beyond what a generation
 * call of the same route allocates on its first use.  The stream is drained before the call returns. */
int lrcn_debug_decode_steps(lrcn_ctx *ctx, lrcn_decode_debug *d);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_DECODE_DEBUG_H */
