/* lrcn_cider.h -- CIDEr-D over token ids on the device: the reward of self-critical caption training (lrcn_amd/scst.py) and the per-epoch
 * dev metric, without the host loop.  Beside the C ABI of include/lrcn.h (which it includes; lrcn.h, its exports and LRCN_ABI_VERSION are
 * unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points.
 *
 * The metric is lrcn_amd/cider.py's, stated over int32 token ids instead of word strings:
 *   n-grams      n = 1..4 of the id sequence, compared as exact int32 tuples (any V up to 2^31 - 1)
 *   document     one per image: df(g) = the number of images whose references contain g
 *   idf(g)       log N - log max(1, df(g)), N = n_images; an n-gram in no reference gets log N.  Both logarithms are taken on the HOST in
 *                double when the handle is made, so the idf values carry the host's bits.
 *   vector       per n, v[g] = count(g) * idf(g); |v| its Euclidean norm
 *   term         per n and reference: sum_g min(v_h[g], v_r[g]) * v_r[g] / (|v_h| |v_r|), skipped when either norm is exactly 0, times
 *                exp(-(l_h - l_r)^2 / (2 * 36)), l = the number of words
 *   score        the mean of the terms over the image's references and over the four n, times 10
 * An empty hypothesis, or an image without references, scores exactly 0.0.
 *
 * Tables (built once by lrcn_cider_create, in C++ on the host, then uploaded; csrc/cider_table.h):
 *   per n        an open-addressing hash table of the distinct n-grams of all references: the full key (n int32) and the idf (double) per
 *                slot, at most half full.  A look-up compares the whole key; the hash only picks where to start.
 *   per n, ref   the reference's distinct n-grams as (slot, count) pairs, and |v_r| (double)
 *   per ref      its length; per image, the list of its references in the order given
 *
 * Kernel: one workgroup (one wave64) per hypothesis.  Its words are staged in LDS; per n the distinct n-grams and their counts come from
 * an all-pairs compare in LDS, each distinct n-gram probes the hash table once, and the image's (slot, count) pairs are read by every lane
 * at wave-uniform addresses, so no load's address depends on another load's result beyond the probe.  All floating-point work is double.
 * Every sum has a fixed order (a lane's own terms in position order, then an xor tree over the 64 lanes; references in their order; n
 * ascending): no floating-point atomics.  A caption's score is a function of the caption, its image and the tables alone -- not of the
 * batch it is scored in, nor of its row.
 *
 * Hypothesis rows have the form lrcn_sample_batch and lrcn_beam_search_batch write: row r is tokens[r*ld ..], bos first, out_len[r]
 * counting bos and a closing eos.  The row's words are positions 1 .. out_len[r]-1, with a trailing eos dropped (a row that ran its
 * nword + 1 steps without eos keeps them all): scst.sample_words on the host.  What the buffer holds from out_len[r] on is not read. */
#ifndef LRCN_CIDER_H
#define LRCN_CIDER_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lrcn_cider lrcn_cider;

#define LRCN_CIDER_MAXWORDS (LRCN_BEAM_MAXLEN - 2)   /* 256: the longest hypothesis, in words */

typedef struct {
    int64_t images, references;
    int64_t ngrams[4];      /* distinct n-grams of all references, n = 1..4 */
    int64_t slots[4];       /* hash-table slots per n (a power of two, at least twice ngrams[n-1]) */
    int64_t ref_entries[4]; /* (slot, count) pairs over all references per n */
    int64_t device_bytes;   /* what the tables hold on the device (the staging of lrcn_cider_score grows with the largest call and is not counted) */
} lrcn_cider_stats_t;

/* All arrays are HOST arrays.  Reference r (0 <= r < n_refs) belongs to image ref_image[r] in [0, n_images) and is
 * ref_tokens[ref_offsets[r] .. ref_offsets[r+1]), ids in [0, V); it may be empty or shorter than n, and an image may have no reference.
 * LRCN_EINVAL: a NULL pointer, n_images < 1, n_refs < 0, V < 1, offsets that do not start at 0 or decrease, 2^29 or more reference words, an
 * image index or a word id out of range. */
int lrcn_cider_create(int device, int n_images, int n_refs, const int32_t *ref_image, const int64_t *ref_offsets, const int32_t *ref_tokens,
                      int V, lrcn_cider **out);
void lrcn_cider_destroy(lrcn_cider *c);
const char *lrcn_cider_last_error(const lrcn_cider *c);   /* c may be NULL: the last creation error */
int lrcn_cider_set_stream(lrcn_cider *c, void *hip_stream); /* hipStream_t; NULL = null stream */
int lrcn_cider_stats(const lrcn_cider *c, lrcn_cider_stats_t *out);

/* tokens [R][ld], out_len [R], image [R] and out [R] are HOST arrays.  The call copies in, runs on the handle's stream, copies out and
 * synchronises.  LRCN_EINVAL before any GPU work, with `out` untouched and the row named in the message: a NULL pointer, R < 1, ld < 2,
 * image[r] outside [0, n_images), out_len[r] outside [2, ld], more than LRCN_CIDER_MAXWORDS words, a word id outside [0, V). */
int lrcn_cider_score(lrcn_cider *c, const int32_t *tokens, int ld, const int32_t *out_len, const int32_t *image, int R, double *out);

/* The same on DEVICE pointers, queued on the handle's stream with no synchronise.  Only the pointers, R and ld are checked on the host.
 * The rows are the caller's contract: a row whose image index is outside [0, n_images), whose out_len is outside [2, ld] or that has
 * more than LRCN_CIDER_MAXWORDS words gets a quiet NaN and touches no table; a word id outside [0, V) is never used as an index, it
 * only matches no reference word (an n-gram holding it counts as one no reference has). */
int lrcn_cider_score_dev(lrcn_cider *c, const int32_t *tokens, int ld, const int32_t *out_len, const int32_t *image, int R, double *out);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_CIDER_H */
