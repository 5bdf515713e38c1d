/* lrcn_constrain.h -- constrained beam search: banned words, a minimum length and no repeated n-grams for the n-best beam of
 * include/lrcn_nbest.h and the diverse beam of include/lrcn_diverse.h (which this header includes; LRCN_ABI_VERSION is unchanged).
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points. */
#ifndef LRCN_CONSTRAIN_H
#define LRCN_CONSTRAIN_H

#include "lrcn_diverse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A constraint set holds three things:
 *   banned           nbanned >= 0 distinct token ids in [1, V).  LRCN_EOS is not allowed here; use min_len for that.  LRCN_BOS and LRCN_UNK
 *                    are allowed.
 *   min_len          >= 0
 *   no_repeat_ngram  >= 0, where 0 means off
 * At step `current` (1-based, as in lrcn_nbest.h), a row's history after bos is w_1 .. w_t with t = current - 1.  Column v is NOT ALLOWED
 * for that row if any of these holds:
 *   1. v is in banned.
 *   2. v == LRCN_EOS and current <= min_len.  So an entry that ends in eos has at least min_len words.
 *   3. With n = no_repeat_ngram >= 1 and t >= n - 1: there is an i in [1, t - n + 1] with w_i .. w_{i+n-2} == w_{t-n+2} .. w_t and
 *      w_{i+n-1} == v.  For n = 1 this is every word already used.  Eos can never be banned by this rule, since it is never in a live
 *      history.
 * The row proposes its K best allowed columns.  They are ranked by float32 logp = (z - max z) - log(sum exp(z - max z)), descending, ties
 * to the lower column.  max and sum are taken over all V columns, banned ones included: the bans do not renormalise, logp stays
 * log softmax(z) over the whole vocabulary, and out_logp remains the model's log p(caption | image) (what lrcn_score_pairs returns).
 * Everything after that is lrcn_nbest.h, or lrcn_diverse.h for G >= 1, unchanged.  That includes the truncated flush at step nword+1,
 * which ignores min_len.  The exact early stop of lrcn_nbest.h stays exact: constraints only remove candidates and logp <= 0 still holds.
 *
 * Feasibility is checked on the host before any GPU work: V - nbanned - 1 - nword >= K.  With that bound every row always has K allowed
 * columns, whatever its history (eos and at most nword history words on top of the list).  Otherwise the call returns LRCN_EINVAL.  Also
 * LRCN_EINVAL: an id outside [1, V), a duplicate id, min_len > nword, negative fields, nbanned > 0 with a NULL list. */
typedef struct { const int32_t *banned; int nbanned; int min_len; int no_repeat_ngram; } lrcn_constraints;

/* G = 0 is the n-best beam (lrcn_beam_nbest_batch), G >= 1 is diverse beam search (lrcn_beam_diverse_batch; lambda is not read at G = 0).
 * Arguments, outputs and errors are those of the two headers; `cons` (host memory, read before the call returns) as above.
 * If cons == NULL, or all three of its parts are empty, the call IS the unconstrained one: the same route, the logits GEMM's fused record
 * epilogue included, and the same bits.
 * Otherwise the step's logits are written as f32 (the route of a nucleus call, lrcn_nucleus.h: the record epilogue is off, the cell
 * epilogue and the tables stay as the router picks them) and one kernel per step (csrc/constrain.hip, one workgroup per row) takes each
 * row's K best allowed columns from them in place of the unconstrained top-K: the normaliser of the unconstrained rows kernel, bit for bit,
 * then a ban bitmap of the row in LDS (the call's list, uploaded once as (V + 31) / 32 words; eos; rule 3 from the row's history on the
 * device), then the same rounds.  The bookkeeping kernels of nbest.hip / diverse.hip run as they are.  With constraints that never bind,
 * the results are those of the unconstrained call on the f32-logits route (LRCN_DECODE_SMAX=0), bit for bit.
 * Cost (tools/constrained_bench.py, profiles/constrained_bench.md; MI355X, bf16, E = H = 1000, V = 10640, 21 steps, 50 banned words,
 * min_len 5, no_repeat_ngram 3, medians of 7 alternating calls): 512 images x K = 10, where lrcn_beam_nbest_batch is on the f32-logits
 * route as well, 12.21 ms against 11.92 ms (+2.4 %, 14 us per step: the kernel alone); 1024 images x K = 5, 11.23 ms against 10.96 ms of
 * lrcn_beam_nbest_batch under LRCN_DECODE_SMAX=0 (+2.5 %) and 9.41 ms on its fused softmax / top-K epilogue, which a constrained call gives
 * up (+19.3 %). */
int lrcn_beam_constrained_batch(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, int K, int G, float lambda, int nword,
                                float alpha, const lrcn_constraints *cons, int32_t *out_tokens, int *out_len, float *out_logp,
                                float *out_score);

/* One step of the same device code on the caller's own device buffers (as lrcn_sample_logits / lrcn_xent_logits): for each of R rows of f32
 * logits [R][ld] the K best allowed columns and their logp into out_idx / out_logp, device [R][K], queued on the context's stream.
 * hist is [R][ld_hist] int32 on the device: position 0 is bos and positions < current are read.  History tokens outside [0, V) are
 * ignored (they never index the bitmap).  Works for any R >= 1 and V >= 1, independent of the model sizes; above V = 16384 the general
 * form runs (log-softmax of the row into scratch owned by the context, -inf over its banned columns, then the plain top-K kernel).
 * Requirements, else LRCN_EINVAL before any GPU work: ld >= V, ld % 4 == 0, 1 <= K <= 32, 1 <= current <= min(ld_hist,
 * LRCN_BEAM_MAXLEN - 1), V - nbanned - 1 - (current - 1) >= K, and what lrcn_constraints requires (min_len is not bounded here).
 * cons == NULL: no constraint; then, and for an empty set, K <= V takes the bound's place. */
int lrcn_constrained_topk_logits(lrcn_ctx *ctx, const float *logits, int64_t ld, int R, int V, int K, const lrcn_constraints *cons,
                                 const int32_t *hist, int64_t ld_hist, int current, int32_t *out_idx, float *out_logp);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_CONSTRAIN_H */
