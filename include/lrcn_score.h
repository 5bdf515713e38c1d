/* lrcn_score.h -- caption scoring (image-caption retrieval, paper section 5.1 / Table 2), beside the C ABI of include/lrcn.h (which it includes;
 * LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points. */
#ifndef LRCN_SCORE_H
#define LRCN_SCORE_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* s(n, m) = sum_{t=0..L_m} log softmax(z_t)[y_t]: image n, caption m, zero initial state, pdrop 0.  Inputs x_0 = bos, x_t = tok(t-1, m);
 * targets y_t = tok(t, m) for t < L_m and y_{L_m} = eos.  This is -(L_m + 1) * lrcn_loss(one row, norm_B = 1, drop = NULL) (lrcn.jl:553-581).
 *
 * feats N x 4096 column-major on the device (normalise beforehand if wanted, lrcn.jl:597).  tokens: HOST [Tmax][M], 0-based, tok(t, m) at
 * t * M + m, entries at t >= lens[m] ignored; lens: host [M], 1 <= lens[m] <= min(Tmax, LRCN_MAX_T).  Two-layer (LRCN-2f) contexts only.
 *   lrcn_score_matrix: scores device f32 N x M column-major, s(n, m) at n + m * N (N * M < 2^31).
 *   lrcn_score_pairs:  scores device f32 [P], scores[p] = s(pair_img[p], pair_cap[p]) (host index arrays).
 * Every bad argument (N, M, P <= 0, NULL pointer, a length outside 1..min(Tmax, 28), a token outside [0, V), a pair index out of range,
 * an n_layers = 1 context) returns LRCN_EINVAL before any GPU work.
 *
 * How: LSTM-1 and P_t = h1_t Wproj depend on the caption only and are computed once per caption (captions sorted by length, descending,
 * stable; the per-token table T1 = Wembed W1x + b1); x_cnn W2x + b2 depends on the image only (the table U2, once per image).  Per pair, only
 * the layer-2 recurrence and the logits remain: the pair rows are ordered by (sorted) caption, so the rows still active at step t are a prefix,
 * and they are cut into pieces of at most max_B rows, each run to its longest caption.  The route is chosen once per PIECE from its row
 * count R (never per step, so a pair's score never mixes routes): from R >= 256 rows (bf16, V >= 256, V % 4 == 0, H2 > 64) the logits GEMM
 * reduces each row to {max, sum exp, z[y]} in its epilogue (GEMM_OUT_SMAX_PICK) and the logits never reach memory; below, in f32 contexts or
 * with LRCN_SCORE_FUSED=0 (read per call) the logits are written and reduced by the training loss kernel.  The gate GEMMs take the decode's
 * cell epilogue under the conditions of the batched beam search's table route (bf16, R >= 256), else GEMM + cell kernel.  Each pair's sum
 * is accumulated in double in step order, and every GEMM of the call takes its ordered form (no float-atomic split-K): a pair's score does
 * not depend on which other pairs share its piece, and a call repeats bit for bit.
 *
 * The work is queued on the context's stream; synchronise before reading scores.  The call waits for the stream before it reuses its scratch
 * and once more after uploading the host arrays.  Scratch: the beam decode's tables (lazily, as lrcn_beam_search_batch) and one device arena of the context, grown (never
 * shrunk) to this call's need and freed by lrcn_destroy: sum_m (L_m + 1) rows of P (h elements of the context's LSTM type each), N x 4H2 f32
 * of U2, 2 x max_B x (h + H2) (padded) of layer-2 operands (zeroed by every call), 2 int32 per caption step, 1 per caption, 3 per pair
 * for lrcn_score_pairs (a matrix piece's row maps are made on the device), and a few max_B-sized arrays.  A score call leaves nothing that a
 * later beam or sample call reads. */
int lrcn_score_matrix(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, const int32_t *tokens, const int *lens, int M, int Tmax,
                      float *scores);
int lrcn_score_pairs(lrcn_ctx *ctx, const float *const params[9], const float *feats, int N, const int32_t *tokens, const int *lens, int M, int Tmax,
                     const int32_t *pair_img, const int32_t *pair_cap, int P, float *scores);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_SCORE_H */
