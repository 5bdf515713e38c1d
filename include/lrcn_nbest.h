/* lrcn_nbest.h -- n-best beam search in log space with length normalisation, beside the C ABI of include/lrcn.h (which it includes;
 * LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement this entry point.
 * lrcn_beam_search_batch stays the reference-faithful beam (lrcn.jl:644-678: float32 probability products, one caption per image). */
#ifndef LRCN_NBEST_H
#define LRCN_NBEST_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N images x K beams, R = N*K <= max_B rows of one batched lrcn() step.  feats N x 4096 column-major on the device (normalise beforehand
 * if wanted, lrcn.jl:597).  Host outputs, entries of an image best first:
 *   out_tokens [N][K][nword + 2]   bos first; ends in eos unless truncated at the length limit; zeros past out_len
 *   out_len    [N][K]              tokens including bos (and eos); 0 = no entry
 *   out_logp   [N][K]              sum of the per-step log-probabilities (may be NULL); -inf for no entry
 *   out_score  [N][K]              out_logp / len^alpha, len = out_len - 1 (may be NULL); -inf for no entry
 * alpha: finite, >= 0 (0 = raw log-likelihood, 1 = per predicted token, as --retrieval_norm mean).
 *
 * The rules, per image (all arithmetic float32 unless stated; lp(L) = (float)pow((double)L, (double)alpha)):
 *   Steps current = 1 .. nword+1.  The image has K slots, each a history (starting [bos]) with a cumulative log-probability cum
 *   (starting 0).  A live slot proposes its K best next words j by logp = (z - max z) - log(sum exp(z - max z)) of its logits z,
 *   ranked by logp descending, ties to the lower column.  At step 1 only slot 0 proposes (every slot is [bos] there, lrcn.jl:662-664).
 *   Candidate (i, j) -- index i*K + j -- has the value cum_i + logp_ij.  All candidates of the image are ranked by value, descending,
 *   ties to the lower candidate index, and walked in rank order: a candidate whose word is eos enters the pool as finished; any other
 *   takes the next free live slot (slot 0 first) as history_i + word with cum = its value.  The walk ends when K slots are full or the
 *   candidates run out; slots left empty are dead (cum = -inf) and propose nothing.  After the walk of step nword+1 the live slots enter
 *   the pool as well, in slot order, truncated (no eos).
 *   An entry of L tokens after bos (L = current for every entry of a step) has score = logp / lp(L).  The pool keeps the K best entries
 *   in order of score, descending: an entry goes after the entries of equal score already there, and enters a full pool only if its
 *   score is strictly greater than the last entry's, which it then displaces.
 *   The image is done after the step where it has no live slot, or where its pool holds K entries and the last pool score is
 *   >= max over live slots of cum / lp(nword+1).  This stop is exact: logp <= 0, so cum never grows, and for cum <= 0, cum / lp(L) is
 *   largest at the longest L = nword+1; no later entry can enter the pool.  The results equal those of running every image to nword+1.
 *
 * How: the batched decode of lrcn_beam_search_batch (the same steps and routes; the logits GEMM's top-K epilogue and its merge, or the
 * rows kernel on f32 logits, return log-probabilities instead of probabilities), then one workgroup per image does the step's ranking,
 * pool and slot bookkeeping on the device; the host polls the done counter every 4 steps.  An image's entries do not depend on which
 * other images share the call on the same route, and a call repeats bit for bit.
 *
 * Bad arguments return LRCN_EINVAL before any GPU work: K outside [1, min(32, V)], N < 1 or N*K > max_B, nword outside
 * [1, LRCN_BEAM_MAXLEN - 2], alpha negative or not finite, a NULL pointer other than out_logp / out_score.
 * Works on f32 and bf16, LRCN-2f and LRCN-1f contexts.  Device state (pool token storage of 2K rows per image, pool lengths, logp and
 * scores, live cum) is allocated on the context on the first call and freed by lrcn_destroy. */
int lrcn_beam_nbest_batch(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, int K, int nword, float alpha,
                          int32_t *out_tokens, int *out_len, float *out_logp, float *out_score);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_NBEST_H */
