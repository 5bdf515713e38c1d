/* lrcn_diverse.h -- diverse beam search (Vijayakumar et al. 2016): the n-best beam of include/lrcn_nbest.h (which this header includes;
 * LRCN_ABI_VERSION is unchanged) split into groups, each group pushed away from the words the groups before it chose at the same step.
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement this entry point. */
#ifndef LRCN_DIVERSE_H
#define LRCN_DIVERSE_H

#include "lrcn_nbest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* N images x K beams, R = N*K <= max_B rows of one batched lrcn() step, as lrcn_beam_nbest_batch.  The K beams of an image are G groups of
 * K' = K / G; group g owns rows n*K + g*K' .. + K'-1.  lambda >= 0 is the strength of the diversity penalty (0: every group repeats
 * group 0).  Host outputs as lrcn_beam_nbest_batch, [N][K] entries, group-major: entry e belongs to group e / K', each group's entries best
 * first, out_len 0 (out_logp / out_score -inf) for no entry.
 *
 * The rules, per image.  Each group is an n-best beam of width K' by the rules of lrcn_nbest.h -- K' slots with cum, at step 1 only the
 * group's slot 0 proposes, the walk (eos to the group's pool, any other word to the group's next free live slot), the pool's insertion
 * rule, lp(L), the flush of truncated entries at step nword+1, float32 arithmetic -- except for how candidates are selected:
 *   At every step the groups are processed in order g = 0 .. G-1.  cnt(w) = the number of live slots that groups 0 .. g-1 of this image
 *   filled with word w at this step (with multiplicity; the last step's slots count before they are flushed; eos never takes a slot and is
 *   never penalised; a dead group adds nothing).
 *   A live row i of group g proposes its K' best words by a_ij = fmaf(-lambda, (float)cnt(w_ij), logp_ij), descending, ties to the lower
 *   column.  Candidate i_local*K' + j has the selection value cum_i + a_ij and the true value cum_i + logp_ij.  The group's candidates are
 *   ranked by selection value, descending, ties to the lower candidate index, and walked in that order.
 *   What is stored is the true value: a new slot's cum, a pool entry's logp and score = logp / lp(L).  out_logp is the model's
 *   log p(caption | image); the penalty steers the search and never enters it.  With cnt = 0, a equals logp bit for bit, so G = 1 is
 *   lrcn_beam_nbest_batch bit for bit at any lambda.
 *   A group is satisfied when its pool holds K' entries and its last pool score is >= max over its live slots of cum / lp(nword+1); its
 *   pool can no longer change (lrcn_nbest.h), and satisfaction is monotone.  A satisfied group keeps running, because its words still
 *   penalise the groups after it.  The image is done after a step where every group is dead (no live slot) or satisfied, or after step
 *   nword+1.  The results equal those of running every image to nword+1.
 *
 * The row's K' penalised best lie inside its K best unpenalised words, which is what the decode step delivers: groups before g fill at
 * most K - K' slots, so at most K - K' distinct words are penalised; of the >= K words ranked above a word outside the top K, at least K'
 * are unpenalised and stay above it (penalties only lower a value), ties included under the (value, column) order.
 *
 * How: the batched decode of lrcn_beam_nbest_batch at full width K with log-probability top-K, then one workgroup per image walks the
 * image's groups in order on the device (csrc/diverse.hip); the host polls the done counter every 4 steps.  An image's entries do not
 * depend on which other images share the call on the same route, and a call repeats bit for bit.
 *
 * Bad arguments return LRCN_EINVAL before any GPU work: everything lrcn_beam_nbest_batch rejects, G < 1, G not dividing K, lambda negative
 * or not finite.  Works on f32 and bf16, LRCN-2f and LRCN-1f contexts.  Device state: the n-best allocations plus one done flag per image. */
int lrcn_beam_diverse_batch(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, int K, int G, float lambda, int nword,
                            float alpha, int32_t *out_tokens, int *out_len, float *out_logp, float *out_score);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_DIVERSE_H */
