/* lrcn_forced.h -- forced-word beam search: captions that must contain given words, for the n-best beam of include/lrcn_nbest.h with the
 * constraints of include/lrcn_constrain.h (which this header includes; LRCN_ABI_VERSION is unchanged).
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points.
 * After Anderson et al. 2017, "Guided open vocabulary image captioning with constrained beam search": the beam becomes a finite-state
 * machine whose states say which of the image's word sets a hypothesis has used, with one beam per state. */
#ifndef LRCN_FORCED_H
#define LRCN_FORCED_H

#include "lrcn_constrain.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LRCN_FORCED_MAXSETS 3
#define LRCN_FORCED_MAXALT  4

/* Sets.  Image n has up to C sets; set c is the non-negative ids among words[n][c][0 .. A): alternatives such as singular and plural.  A set
 *   with no id is absent for that image.  Ids lie in [1, V) (the range of `banned`: no eos), no id occurs twice within one image (an
 *   image's sets are disjoint), and no id is in cons->banned.
 * State.  The state of a history w_1 .. w_t is the bitmask m whose bit c is set iff some w_i is in set c of the image.  full_n is the mask
 *   of the image's present sets; a hypothesis is ACCEPTING iff m == full_n.
 * Banks.  S = 2^C.  The image owns S * K rows; bank b is rows n*S*K + b*K .. + K-1 and holds only hypotheses of state b.  Banks whose mask
 *   is not a subset of full_n stay dead.
 * A step (current = 1 .. nword+1; float32 as in lrcn_nbest.h).  At step 1 only row 0 of bank 0 is live.  A live row i has cum_i and state
 *   b; its logp is taken over all V columns and never renormalised.
 *   Allowed columns   rules 1-3 of lrcn_constrain.h (when cons is non-empty), and rule 4: eos is not allowed unless the row is accepting.
 *   Stay proposals    the row's K best allowed columns that are not a word of a present, unsatisfied set of this row, by logp descending,
 *                     ties to the lower column.  Target: bank b.  Words of satisfied sets are ordinary columns.
 *   Move proposals    for each present set c not in b, ascending, and each alternative a, ascending, whose word is allowed by rules 1-3:
 *                     target bank b | 1<<c, value cum_i + logp[word].
 *   Candidate index   within the image, i*(K + C*A) + j for stay proposal j and i*(K + C*A) + K + c*A + a for a move.
 *   Walk              every bank b' ranks the candidates that target it -- the stay proposals of its own rows and the moves from the banks
 *                     one bit below it -- by value descending, ties to the lower candidate index.  An eos candidate enters the image's ONE
 *                     pool (K entries; the insertion rule, lp(L) and score of lrcn_nbest.h); any other word takes the bank's next free slot
 *                     with cum = its value.  The walk ends when the bank's K slots are full or its candidates run out.  Eos can only
 *                     occur in bank full_n.
 *   Independence      banks do not interact within a step: all candidates come from the state before the step.
 *   Flush             after the walk of step nword+1 the new slots of bank full_n enter the pool truncated, in slot order; the other
 *                     banks' slots are dropped.
 *   Done              after a step with no live slot in any bank, or when the pool holds K entries and the last pool score is >= max over
 *                     all new live slots of all banks of cum / lp(nword+1).  Exact by the argument of lrcn_nbest.h: a live hypothesis of
 *                     any bank can only finish later, with a cum that has not grown.
 *   An image whose sets were never met returns fewer than K entries, possibly none (out_len 0, -inf).  out_logp stays the model's
 *   log p(caption | image).
 * Why one top-K per row is exact: a row's candidates for its own bank are its stay proposals only, and the bank takes at most K of them
 *   (K slots, plus eos, which is one column), so the row's K best stay columns -- and eos among them where it ranks -- hold every candidate
 *   the walk can reach from that row; moves are at most C*A named columns, all listed.
 *
 * Checked on the host before any GPU work, else LRCN_EINVAL: everything lrcn_beam_nbest_batch and lrcn_constraints check; 0 <= C <= 3, and
 * 1 <= A <= 4 and words != NULL when C > 0; S*K <= 32 and N*S*K <= max_B; nword >= C; the id rules above; feasibility
 * V - nbanned - 1 - nword - C*A >= K (then every row has K stay columns whatever its history: no kernel has a "fewer than K" case).
 * forced == NULL or C == 0: the call IS lrcn_beam_constrained_batch(.., G = 0, ..): the same route, the fused record epilogue included, and
 * the same bits.
 *
 * How: the decode of lrcn_beam_constrained_batch on N*S*K rows (f32 logits, the cell epilogue and the tables as the router picks them for
 * that row count).  Per step one kernel per row (csrc/constrain.hip, forced_topk_rows_kernel: the constrained kernel's normaliser, bit for
 * bit; the row's state from its history in LDS; the move values read from the row; then the unsatisfied sets' words join the ban bitmap and
 * the same rounds run) and one workgroup per image (csrc/forced.hip) that walks the banks, keeps the pool and writes parents -- which may
 * point into another bank of the image -- tokens, histories and results.  The word table is uploaded once per call behind the ban bitmap.
 * Cost (tools/forced_bench.py, profiles/forced_bench.md; MI355X, bf16, E = H = 1000, V = 10640, 21 steps, no early stop, 256 images, K = 5,
 * sets of 2 words, medians of 7 alternating calls, against lrcn_beam_constrained_batch on the same f32-logits route): C = 1, 2560 rows, 6.89
 * ms against 7.17 ms at width 10 (the same rows, x 0.96) and 4.05 ms at width 5 (the same output, x 1.70); C = 2, 5120 rows, 11.96 ms
 * against 14.61 ms at width 20 (x 0.82) and 4.05 ms at width 5 (x 2.95).  A forced call costs its rows: the decode of S * K rows per image,
 * less what the narrower top-K (K rounds, not S * K) and bookkeeping save. */
typedef struct { const int32_t *words; int C; int A; } lrcn_forced;   /* words: host, [N][C][A], -1 = no word */

/* outputs [N][K], as lrcn_nbest.h */
int lrcn_beam_forced_batch(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, int K, int nword, float alpha,
                           const lrcn_constraints *cons, const lrcn_forced *forced, int32_t *out_tokens, int *out_len, float *out_logp,
                           float *out_score);

/* One step of the top-K kernel on the caller's own device logits [R][ld], one row per "image": words is host [R][C][A].  Outputs on the
 * device: out_idx / out_logp [R][K] the stay proposals, out_move_logp [R][C*A] the move values (-inf: the word is absent, its set is
 * satisfied, or rules 1-3 ban it), out_state [R] the row's state.  Queued on the context's stream.  Above V = 16384 the general form runs
 * (log-softmax into scratch owned by the context, one kernel that gathers the move values and writes -inf by the same rules, the plain
 * top-K).  Requirements, else LRCN_EINVAL before any GPU work: those of lrcn_constrained_topk_logits with C*A added to the feasibility
 * bound, V - nbanned - 1 - (current - 1) - C*A >= K (asked for an empty constraint set as well), and the C, A and id rules above. */
int lrcn_forced_topk_logits(lrcn_ctx *ctx, const float *logits, int64_t ld, int R, int V, int K, const lrcn_constraints *cons,
                            const int32_t *words, int C, int A, const int32_t *hist, int64_t ld_hist, int current, int32_t *out_idx,
                            float *out_logp, float *out_move_logp, int32_t *out_state);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_FORCED_H */
