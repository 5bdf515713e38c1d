/* lrcn_nucleus.h -- nucleus (top-p) sampling and top_k of any width for the sampled caption decode, beside the C ABI of include/lrcn.h
 * (which it includes; LRCN_ABI_VERSION is unchanged) and lrcn_sample.h (whose lrcn_sample_batch stays as it is).
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points.
 *
 * The definition.  One row of f32 logits z[0..V), a temperature T > 0, top_k in [0, V], top_p in (0, 1]:
 *   rank order    larger z first, lower column first among equal z (the rule of lrcn_sample.h; -0 and +0 are equal)
 *   A_k           the first top_k columns in rank order; top_k = 0 means all V
 *   weights       w_j = exp((z_j - max z) / T) for j in A_k, W = sum of them: the nucleus is taken on the distribution renormalised after the
 *                 top-k cut
 *   n             the smallest n >= 1 such that the first n columns of A_k in rank order have sum w >= top_p * W
 *   admitted set  those n columns; columns that share the boundary value enter in column order, only as many as are needed
 *   top_p = 1     no mass is computed at all and n = |A_k|
 * The draw is that of lrcn_sample.h: tok = argmax_j (z_j / T + g_j) over the admitted columns with z_j >= max z - 20 T (no other column can
 * win), g_j from Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (j >> 2, current, s, i).  The reported log-probability is
 * log softmax(z)[tok] over the WHOLE vocabulary at temperature 1.  T = 0 is greedy: top_k and top_p are accepted and have no effect (the
 * admitted set is the whole row, n = V).
 *
 * The sums are f32 and run in one fixed order (per-thread partials in column order, then a fixed shuffle and LDS tree; no float atomics), so
 * two identical calls return identical tokens and identical n.  Against the exact (real-number) definition the boundary can move only where a
 * prefix share lies within about V * 2^-24 (relative) of top_p.
 *
 * Cost.  The selection needs the whole row, so a nucleus call (top_p < 1 or top_k > 32) takes the plain-logits route of the batched decode
 * -- the logits GEMM writes f32 logits, what LRCN_DECODE_SMAX=0 selects for lrcn_sample_batch -- and pays that route plus the selection:
 * 32 block-wide rounds over the row for the top_k cut and 32 for the mass.  Measured (profiles/nucleus_bench.md: MI355X, 1024 images x 5
 * samples, V = 10640, bf16, 9 steps): 248 k captions/s at top_p 0.9 and 354 k at top_k 100 against 636 k for top_k 0 on the same route; per
 * step the selection and draw take 1.60 ms resp. 0.91 ms, the logits GEMM 0.27 ms. */
#ifndef LRCN_NUCLEUS_H
#define LRCN_NUCLEUS_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lrcn_sample_batch (lrcn_sample.h: the same arguments, outputs, row order and stop rule) with 0 <= top_k <= V and 0 < top_p <= 1.
 * out_count: host [N][S][nword + 1], may be NULL: the admitted set's size n at step current = 1 .. nword+1 of every row, 0 at the steps
 * after the row has finished.  With top_p == 1 and top_k <= 32 this IS lrcn_sample_batch (the same code path on all three of its routes,
 * bit for bit; out_count then holds |A_k| at every live step).  Otherwise the step's logits go to f32 (the cell epilogue and the tables stay
 * as the router picks them) and one workgroup per row selects and draws.  Bad arguments (top_p NaN, <= 0 or > 1; top_k < 0 or > V; those of
 * lrcn_sample_batch) return LRCN_EINVAL before any GPU work. */
int lrcn_sample_batch_p(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, int S, int nword,
                        float temperature, int top_k, float top_p, uint64_t seed,
                        int32_t *out_tokens, int *out_len, float *out_logp, int32_t *out_count);

/* One step of the same selection and draw on the caller's DEVICE logits: row r (image r / S, sample r % S) starts at logits + r*ld, ld >= V;
 * any R >= 1, V >= 1, S >= 1, independent of the context's model sizes.  Device outputs [R]: out_tok, out_logp (may be NULL), out_count
 * (may be NULL).  Queued on the context's stream (lrcn_sync to wait).  The same device code as lrcn_sample_batch_p's step. */
int lrcn_sample_logits(lrcn_ctx *ctx, const float *logits, int64_t ld, int R, int V, int S, int current,
                       float temperature, int top_k, float top_p, uint64_t seed,
                       int32_t *out_tok, float *out_logp, int32_t *out_count);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_NUCLEUS_H */
