/* lrcn_sample.h -- sampled caption generation, beside the C ABI of include/lrcn.h (which it includes; LRCN_ABI_VERSION is unchanged).
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement this entry point. */
#ifndef LRCN_SAMPLE_H
#define LRCN_SAMPLE_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sampled generation (the sample() path of lrcn.jl:613-621, 680-687) for N images x S samples per image, R = N*S <= max_B rows of one
 * batched lrcn() step.  feats N x 4096 column-major (normalise beforehand if wanted, lrcn.jl:597).  Host outputs:
 * out_tokens [N][S][nword + 2] (bos first, the same length / eos convention as lrcn_beam_search_batch), out_len [N][S],
 * out_logp [N][S] (may be NULL): sum over the emitted tokens after bos of log softmax(logits)[token] at temperature 1, f32.
 * temperature 0 = greedy (lowest column wins a tie); top_k 0 = the whole vocabulary, else 1 <= top_k <= min(32, V).
 *
 * Row r = i*S + s is its own hypothesis (its state never moves to another row) and stops after it emits eos; steps run
 * current = 1 .. nword+1.  Each step draws tok = argmax_j (z_j / T + g_j) (Gumbel-max, the distribution of softmax(z / T)), j over the
 * top_k largest logits z (ties at the boundary: lower column) or all of them, with g_j = -log(-log(u)), u = ((x >> 9) + 0.5) * 2^-23 in
 * float32, x = word (j & 3) of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (j >> 2, current, s, i).  So the samples
 * of image i depend only on (seed, i, s, current, j), not on which other images share the call.  At T = 0 the result equals
 * lrcn_beam_search_batch with K = 1.  Bad arguments return LRCN_EINVAL before any GPU work. */
int lrcn_sample_batch(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, int S, int nword,
                      float temperature, int top_k, uint64_t seed, int32_t *out_tokens, int *out_len, float *out_logp);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_SAMPLE_H */
