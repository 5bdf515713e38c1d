/* lrcn_ensemble.h -- ensemble beam search: M caption models decode as one.  Every step the members' next-word distributions are mixed
 * into one row per hypothesis, and the n-best beam of include/lrcn_nbest.h, the diverse beam of include/lrcn_diverse.h and the constraints
 * of include/lrcn_constrain.h (which this header includes; LRCN_ABI_VERSION is unchanged) run on the mixture as they run on one model.
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points. */
#ifndef LRCN_ENSEMBLE_H
#define LRCN_ENSEMBLE_H

#include "lrcn_constrain.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LRCN_ENSEMBLE_MAX 8
#define LRCN_ENSEMBLE_PROB 0    /* arithmetic mean of the members' distributions */
#define LRCN_ENSEMBLE_LOGPROB 1 /* geometric mean: weighted sum of their log-probabilities */

/* There are M members, 1 <= M <= LRCN_ENSEMBLE_MAX.  Member m has logits z_m for a row and, in float32,
 *   lp_m[v] = (z_m[v] - max z_m) - log(sum exp(z_m - max z_m))          over all V columns.
 * The weights w_m are positive and finite on input; the host normalises them in double to sum 1 and then rounds to float.  weights == NULL
 * means uniform.  The MIXTURE ROW x of a row is, in float32:
 *   LRCN_ENSEMBLE_PROB     x[v] = mx[v] + log(sum_m w_m * exp(lp_m[v] - mx[v])),  mx[v] = max_m lp_m[v].  The per-column maximum keeps a
 *                          column finite that is improbable in every member.  The terms are summed in member order.
 *   LRCN_ENSEMBLE_LOGPROB  x[v] = sum_m w_m * lp_m[v], summed in member order and not renormalised.
 * A mixture row is a LOGIT row.  The selection that follows treats it exactly as it treats one model's logits:
 * logp = (x - max x) - log(sum exp(x - max x)), the constraints on the allowed columns, the K best descending with ties to the lower
 * column.  In PROB mode this renormalisation moves x by rounding only; in LOGPROB mode it is what normalises the geometric mean.
 * Everything behind the proposal is lrcn_nbest.h, lrcn_diverse.h and lrcn_constrain.h unchanged: the pool, length normalisation, the exact
 * early stop (it needs logp <= 0 only, which still holds), the diversity penalty, the three constraint rules.  out_logp is the sum of the
 * mixture's per-step log-probabilities.
 *
 * ctx[0] is the leader: it owns the histories, the pool, the done flags, the constraint bitmap, the results and a mixture buffer
 * [max_B][ldV] f32 (allocated on the first ensemble call, freed by lrcn_destroy).  Every member is a whole context of its own with its own
 * parameter set: members may differ in E, H1, H2, the number of layers and the dtype.  They must share V, the device and the stream handle,
 * and each needs max_B >= N*K.  One feats, N x 4096 as for lrcn_beam_nbest_batch, serves all members.
 * Per step every member runs its own decode step on the route its own sizes pick (f32 logits: the record epilogue is off, as for a
 * constrained call), ONE launch (csrc/ensemble.hip, one workgroup per row) mixes the M logit rows, the constrained top-K kernel and the
 * leader's bookkeeping kernel run on the mixture, and the leader's parents and next tokens are copied to the other members on the device.
 * No host wait is added to those of lrcn_beam_constrained_batch.
 * Cost (tools/ensemble_bench.py, profiles/ensemble_bench.md; MI355X, bf16, E = H = 1000, V = 10640, 21 steps, PROB, medians of 7 alternating
 * calls) against M single-model calls on the same f32-logits route: 512 images x K = 10, M = 2 26.00 ms against 2 x 12.16 ms (x 1.07), M = 4
 * 47.16 ms against 4 x 12.16 ms (x 0.97); 1024 images x K = 5, M = 2 25.05 ms against 2 x 11.15 ms (x 1.12), M = 4 46.13 ms against 4 x 11.15
 * ms (x 1.03).
 * M == 1 IS lrcn_beam_constrained_batch on ctx[0], bit for bit (a weight, if given, must still be valid).
 * Outputs are those of lrcn_beam_constrained_batch.
 * LRCN_EINVAL before any GPU work, with a message in ctx[0]'s last error that names the member: M outside [1, LRCN_ENSEMBLE_MAX], a NULL
 * context or parameter set, a weight that is not positive and finite, a mode other than the two above, members that differ in V, device or
 * stream, a member's max_B < N*K, a context given twice, and everything lrcn_beam_constrained_batch rejects. */
int lrcn_beam_ensemble_batch(lrcn_ctx *const ctx[], const float *const *params[], int M, const float *weights, int mode, const float *feats,
                             int N, int K, int G, float lambda, int nword, float alpha, const lrcn_constraints *cons, int32_t *out_tokens,
                             int *out_len, float *out_logp, float *out_score);

/* The mix kernel alone on the caller's own device buffers (as lrcn_constrained_topk_logits is for its kernel): out [R][ld_out] takes the
 * mixture rows of logits[m] [R][ld[m]], m < M, queued on the context's stream.  Independent of the context's model sizes; any R >= 1,
 * V >= 1, ld[m] >= V, ld_out >= V, any alignment (16-byte loads and stores where a buffer's base and leading dimension allow, scalar ones
 * elsewhere).  `out` must not overlap an input.  Inputs must be finite.  A call repeats bit for bit.
 * LRCN_EINVAL: a NULL pointer, M, weights or mode as above, R or V < 1, a leading dimension below V. */
int lrcn_ensemble_mix_logits(lrcn_ctx *ctx, const float *const logits[], const int64_t ld[], int M, const float *weights, int mode, int R, int V,
                             float *out, int64_t ld_out);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_ENSEMBLE_H */
