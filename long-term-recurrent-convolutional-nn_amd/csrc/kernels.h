// kernels.h -- launchers of the non-GEMM kernels of liblrcn_hip (gfx950), one section per .hip file that defines them, in the Makefile's
// order.  dtype: GEMM_T_F32 / GEMM_T_BF16 selects the element type "T" of activation/shadow buffers; everything marked f32 is always float.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct DropSpec {
    float p;            // drop probability (0 = identity)
    uint64_t seed;      // counter-hash key
    const float *mask;  // caller-supplied multipliers ((T+1) blocks of B x ncols, column-major) or NULL
    int which;          // 1 = the mask of lrcn.jl:542, 2 = the mask of lrcn.jl:547
};

// ---- lstm_fused.hip ----
// Small-batch fused recurrent steps (lstm_fused.hip; bf16, B <= 64): one launch = the recurrent GEMM of a timestep + the cell
// update (forward) / the dh GEMM of step s + the cell backward of step s-1.
bool lstm_fused_eligible(int dtype, int B, int H, int64_t ldh, int64_t ld4);
hipError_t launch_lstm_rec_fwd(hipStream_t st, const void *h_prev, int64_t ldh, const void *Wh, const float *Gx, const float *c_prev, int B,
                               int H, void *acts, int64_t ld_a, float *c_new, void *h_new, const void *zero_page, bool alone = false);
hipError_t launch_lstm_rec_bwd(hipStream_t st, const void *dz_s, int64_t ld4, const void *WhT, const void *acts, const float *c_prev,
                               const float *c_new, const float *dh_ext, float *dc, int B, int H, void *dz_out, const void *zero_page,
                               bool alone = false);
// alone: nothing else runs on the GPU beside the LSTM step -- up to LRCN_LSTM_REC2 rows (default 64) the step kernels then take
// their 8-units-per-workgroup forms (125 / 250 workgroups instead of 63; lstm_fused.hip)

// ---- conv11.hip ----
// conv1_1 + preprocessing fused, bf16 (conv11.hip): src = uint8 crops img[n][row][col][3] or float (S,S,3,N);
// w [64][32] bf16 (k = tap*3+c), out NHWC bf16 [n][y][x][64] with bias + ReLU.
void k_conv11_fused(hipStream_t st, int src_is_u8, const void *src, int N, int S, float m0, float m1, float m2, const void *w,
                    const float *bias, void *out);

// ---- fp8.hip: OCP e4m3 plumbing of the VGG convolution stack ----
void k_quant_conv_w_fp8(hipStream_t st, const float *w, int Cin, int Cout, void *out, float *sw);
void k_amax(hipStream_t st, const void *x, int64_t n, float *out);  // bf16 x: atomic max of |x| into *out (caller zeroes)
void k_cast_bf16_fp8(hipStream_t st, const void *x, int64_t n, float inv_scale, void *out);  // n % 8 == 0
void k_cast_fp8_bf16(hipStream_t st, const void *x, int64_t n, float scale, void *out);
void k_fp8_epilogue_params(hipStream_t st, const float *b, const float *sw, int Cout, float sa_in, float sa_out, float *escale, float *ebias);
void k_ref_to_nhwc_fp8(hipStream_t st, const float *x, int W, int H, int C, int N, float inv_scale, void *out);
void k_nhwc_fp8_to_ref(hipStream_t st, const void *in, int W, int H, int C, int N, float scale, float *out);

// ---- kernels.hip: what more than one model file launches ----
// Xemb[m][e] = WembT[tok_in[m]][e] * dropmask   (lrcn.jl:556/569 gather + :542 dropout), m = s*B+b.
void k_embed_gather(hipStream_t st, int dtype, const void *wembT, int64_t ld_w, const int32_t *tok_in, int S, int B,
                    int E, DropSpec d, void *xemb, int64_t ld_x);

// LSTM cell, one timestep (lrcn.jl:531-536).  G f32 [B][4H] = pre-activations incl. bias; c_prev f32 [B][H] or NULL.
// Writes activated gates [f|i|o|g] (T), c_new (f32), h_new (T) and optionally h_new as f32.
void k_lstm_fwd(hipStream_t st, int dtype, const float *G, int64_t ld_g, const float *c_prev, int B, int H, void *acts,
                int64_t ld_a, float *c_new, void *h_new, int64_t ld_h, float *h_new_f32);
// Reverse of the cell.  dh_a (+ dh_b, may be NULL) f32 [B][H]; dc f32 [B][H] is read and replaced by
// dc_prev.  Writes dZ (T) [B][4H].
void k_lstm_bwd(hipStream_t st, int dtype, const void *acts, int64_t ld_a, const float *c_prev, const float *c_new,
                const float *dh_a, int64_t ld_dha, float *dh_b, int dh_b_read, float *dc, int dc_zero, int B, int H, void *dz,
                int64_t ld_dz, int nslab = 0);   // nslab > 0: dh_b = [nslab][B][H] partial sums, summed here

// X2[m][j<nl] *= mask ; X2[m][nl+j] = xcnn[b][j] * mask (j < nr); mask over nl+nr columns      (lrcn.jl:546-547: nl = nr = h;
// LRCN-1f: nl = E, nr = h)
// s0: the step of x2's first row block (the multipliers are those of steps s0 .. s0 + S - 1; the stepwise forward of scheduled sampling)
void k_concat_x2(hipStream_t st, int dtype, void *x2, int64_t ld_x2, const float *xcnn, int64_t ld_xc, int S, int B,
                 int nl, int nr, DropSpec d, int s0 = 0);

// out[c][r + shift] = in[r][c] (0<=r<R, 0<=c<C), out[c][0..shift) = 0.  in_f32/out types: in is f32 if in_f32 else T;
// out is always T.   (builds the K-contiguous transposed operands of the weight-gradient GEMMs)
void k_transpose(hipStream_t st, int dtype, int in_f32, const void *in, int64_t ld_in, int R, int C, void *out,
                 int64_t ld_out, int shift);
// out_f32[c][r] = in[r][c], f32 -> f32 (boundary layout changes)
void k_transpose_f32(hipStream_t st, const float *in, int64_t ld_in, int R, int C, float *out, int64_t ld_out);
// out[r][c] = (T) in[r*ld_in + c]  (f32 -> T copy of a sub-matrix; pads [C, ld_out) with zeros)
void k_cast_rows(hipStream_t st, int dtype, const float *in, int64_t ld_in, int R, int C, void *out, int64_t ld_out);

// db[n] = sum_m Z[m][n]   (Z is T [M][ld]); f32 output, overwritten.
// deterministic: one slab of rows per column block (no atomics between slabs)
void k_colsum(hipStream_t st, int dtype, const void *z, int64_t ld, int M, int N, float *out, bool deterministic = false);
// Several T -> T transposes in one launch: dst[c][shift + r] = src[r][c]; columns [0, shift) and [R + shift, ld_dst) of every
// destination row are written as zeros (K padding of the GEMM that consumes it).  R == 0 zero-fills the C destination rows.
#define TR_MAX 4
struct TrDesc {
    const void *src;
    void *dst;
    int64_t ld_src, ld_dst;
    int R, C, shift, tile0;
};
struct TrPlan {
    TrDesc d[TR_MAX];
    int n;
};
void k_transpose_multi(hipStream_t st, int dtype, TrPlan &plan);

// xavier-uniform / constant fill (initweights, lrcn.jl:489-510)
void k_init_uniform(hipStream_t st, float *w, int64_t n, float scale, uint64_t seed, int tensor);
void k_fill(hipStream_t st, float *w, int64_t n, float v);

// ---- xent.hip: the loss stage (train.hip, decode.hip's unfused scoring) ----
// Row-wise log-softmax + target pick + (optional) dlogits = (softmax - onehot) * scale   (lrcn.jl:562-567 and dual), in the form that the
// call's members select (k_softmax_xent derives it, in this order):
//   eps > 0   SMOOTH (include/lrcn_smooth.h), weighted exactly when row_w is non-NULL: the target distribution is (1 - eps) onehot(t) + eps / V,
//               term = w ((1 - eps) ll + eps u),  ll = (z_t - max) - log(sum exp),  u = sum_v (z_v - max) / V - log(sum exp)
//               dlog_v = (softmax_v - (1 - eps) [v == t] - eps / V) * (scale * w),  w = row_w[m % B], or 1 without row_w
//             the smoothed term goes where the other forms put theirs and the plain w * ll likewise into ll_rows[m], else *ll_sum.
//   row_w     WEIGHTED (include/lrcn_weighted.h): row m belongs to caption b = m % B.  row_w[b] == 0 makes the row inactive; otherwise its
//             dlog row is (softmax - onehot) * (scale * row_w[b]) and its term row_w[b] * log p(target), in double.
//   masked    MASKED (include/lrcn_varlen.h): a row with tgt[m] < 0 (written by k_build_tokens_var) is inactive -- it adds no loss term,
//             gets rows[m] = 0 (and ll_rows[m] = 0) and an all-zero dlog row, and its logits are not read.
//   else      PLAIN: every row active, term = z_t - (max + log(sum exp)).
// A row's term goes to rows[m] if rows is given (LRCN_OPT_DETERMINISTIC), else as a double atomic into *sum; rows and sum both given: one
// workgroup then adds the rows to *sum in a fixed order (ll_rows and ll_sum the same).  The smooth forms leave a NULL destination out
// (rows with a NULL sum: written and not summed, lrcn_xent_logits); the others need one of sum and rows.
struct XentCall {
    const float *logits; int64_t ld_l;     // f32 [M][ld_l]
    const int32_t *tgt;  int M, V;
    float scale;
    void *dlog; int64_t ld_d;              // T [M][ld_d], or NULL
    double *sum, *rows;                    // accumulator of the terms; their per-row slots [M]
    bool masked;                           // tgt[m] < 0 marks an inactive row
    const float *row_w; int B;             // device f32 [B] or NULL (needs masked)
    float eps;                             // > 0: label smoothing (needs masked)
    double *ll_sum, *ll_rows;              // smoothing's second accumulator; NULL without eps
};
void k_softmax_xent(hipStream_t st, int dtype, const XentCall &x);
// out[m] = tgt[m] in [0, V) ? tgt[m] : -1 (lrcn_xent_logits: a caller's target can never index outside its logits row)
void k_xent_targets(hipStream_t st, const int32_t *tgt, int M, int V, int32_t *out);

// ---- train_kernels.hip: the training step (train.hip, update.hip) ----
// tok_in[s][b] = bos (s==0) | tokens[s-1][b];  tok_tgt[s][b] = tokens[s][b] (s<T) | eos.   (lrcn.jl:556,565,569,576)
void k_build_tokens(hipStream_t st, const int32_t *tokens, int T, int B, int V, int32_t *tok_in, int32_t *tok_tgt, double *zero_acc);
// Per-row lengths (device int32 [B], 0 <= lens[b] <= T): row b's step s is active for s <= lens[b] -- tok_in / tok_tgt as above with
// lens[b] in T's place.  An inactive step gets tok_in = eos (a valid row of the embedding gather) and tok_tgt = -1, the marker
// k_softmax_xent's masked forms skip by; tokens[t][b] at t >= lens[b] is never read, so padding cannot raise the sticky flag.
void k_build_tokens_var(hipStream_t st, const int32_t *tokens, const int32_t *lens, int T, int B, int V, int32_t *tok_in, int32_t *tok_tgt,
                        double *zero_acc);
// dWembed(tok, e) += dXemb[m][e] * dropmask   (AutoGrad dual of the gather; Wembed is V x E column-major f32),
// through an E-contiguous staging array stage[V][ld_s] (f32, all zero on entry and on exit): coalesced atomics per token row,
// then one dense transpose that writes EVERY element of dwembed (no memset needed).  sort_keys != NULL ((T+1)*B <= 8192 keys of scratch):
// the rows of a token are added in a fixed order by plain stores instead (LRCN_OPT_DETERMINISTIC); false = more than 8192 rows, nothing
// was launched.
bool k_embed_scatter_rm(hipStream_t st, const float *dxemb, int64_t ld_dx, const int32_t *tok_in, int S, int B, int E, int V, DropSpec d,
                        float *stage, int64_t ld_s, float *dwembed, unsigned long long *sort_keys);
// the rows of dXemb (dropout multiplier applied) E-contiguous into out [S*B][E]: a rank's share of the sparse embedding-gradient exchange
void k_embed_rows_export(hipStream_t st, const float *dxemb, int64_t ld_dx, int S, int B, int E, DropSpec d, float *out);

// Scheduled sampling (include/lrcn_sched.h): the input of step s_next, decided and gathered after step s_next - 1's logits.
struct SchedNext {
    const float *logits;   // f32 [B][ld_l]: the logits rows of step s_next - 1
    int64_t ld_l;
    int V, B, s_next;
    const int32_t *lens;   // device [B]
    float eps, temp;
    uint32_t k0, k1;       // seed & 0xffffffff, seed >> 32
    uint32_t row0;         // (uint32) index of row 0 in the global batch
    int32_t *tok_in;       // [(T+1) B]: row s_next*B + b holds the gold word (eos past the row's end) and receives a drawn one
    const void *wembT;     // T [V][ld_w]
    int64_t ld_w;
    int E;
    DropSpec d;            // the multipliers of the gather (step s_next), or none
    void *xemb;            // T [(T+1) B][ld_x]: row s_next*B + b is written
    int64_t ld_x;
    long long *cnt;        // [2]: += coins taken, += coins fired
};
// One 256-thread workgroup per row b: past the row's end the eos row is gathered; else the coin is taken and, only where it fires, the
// logits row is read (staged in LDS up to V = 15360) and the word drawn as k_sample_rows draws with top_k = 0.
void k_sched_next_input(hipStream_t st, int dtype, const SchedNext &a);
// cnt[0] = eligible, cnt[1] = drawn (the counters of lrcn_sched_stats at the start of a call)
void k_sched_stats_set(hipStream_t st, long long *cnt, long long eligible, long long drawn);

// dX2[m][j] *= mask (all nl+nr columns, in place);  dxcnn[b][j] = sum_s dX2[s*B+b][nl+j]
void k_dx2_mask_reduce(hipStream_t st, int dtype, void *dx2, int64_t ld, int S, int B, int nl, int nr, DropSpec d,
                       float *dxcnn, int64_t ld_dxc);

// One launch for all shadow weights: parameter memory image src[R][C] (f32, C contiguous) -> direct copies split at column cs
// (dA[r][c] | dB[r][c - cs]) and transposed copies (tA[c][r] | tB[c - cs][r]) in T; NULL destinations are skipped.  Padding
// columns of the destinations are left as they are (zero since allocation).
#define PREP_MAX 12
struct ClipCtl;  // below: the control block of gradient-norm clipping
struct PrepDesc {
    const float *src;
    // k_adam_shadows only: the tensor's gradient and Adam moments (memory images like src, which is then also written)
    const float *g;
    float *m, *v;
    int R, C, cs;
    void *dA, *dB, *tA, *tB;
    int64_t ldA, ldB, ldtA, ldtB;
    int tile0;
    // optional third direct copy of the B side with the ROWS in (unit, gate)-interleaved order: source row g*giH + u -> row 4u + g
    // (the recurrent weights of gemm_8p.hip's LSTM_FWD epilogue); NULL = none
    void *dG;
    int64_t ldG;
    int giH;
    // permH > 0: the DIRECT copies dA / dB are written with their rows in (unit, gate)-interleaved order (source row g*permH + u -> row
    // 4u + g): the concatenated [x | h] decode weights of the cell-epilogue decode step (round 5)
    int permH;
};
struct PrepPlan {
    PrepDesc d[PREP_MAX];
    int n;
    int total;                      // tiles of all descriptors (set by the launchers)
    int grid_cap;                   // always 0 (a capped update grid lost its measurement, DESIGN_HISTORY.md); kept for the kernels' argument layout
    float lr, b1, b2, eps, c1, c2;  // k_adam_shadows
    const ClipCtl *clip;            // k_adam_shadows: non-NULL = the clipped form (reads scale / skip; see ClipCtl)
};
void k_prepare_weights(hipStream_t st, int dtype, PrepPlan &plan);
// update! (lrcn.jl:394) and the NEXT step's shadow weights in one pass over the parameters: every descriptor's src / g / m / v are
// updated exactly as k_adam does (same arithmetic, element by element) and the new values are written to the descriptor's shadow
// destinations.  Descriptors without destinations (the biases: R = 1) are plain Adam.
// plan.clip != NULL: the clipped form -- every gradient element is multiplied by clip->scale first (its own float multiply); with
// clip->skip set w, m and v are not written, and the shadows are still made, from the unchanged parameters.
void k_adam_shadows(hipStream_t st, int dtype, PrepPlan &plan, int step, float lr, float b1, float b2, float eps);

struct AdamTensors {
    float *w[9];
    const float *g[9];
    float *m[9];
    float *v[9];
    int64_t n[9];
};
// update! with Adam (lrcn.jl:394; Knet defaults), all 9 tensors in one launch.
// clip != NULL: the clipped form (g[i] * clip->scale as its own float multiply; nothing is written when clip->skip is set).
void k_adam(hipStream_t st, const AdamTensors &t, int step, float lr, float b1, float b2, float eps, const ClipCtl *clip = nullptr);

// ---- global gradient-norm clipping (include/lrcn_clip.h) ----
// The context's control block in device memory.  slot[k]: sum of squares of gradient tensor k (or of a rank's slice of group k);
// k_clip_set turns the first n_slots of them into norm / scale / skip and bumps the counters.
struct ClipCtl {
    double slot[9];
    double norm;
    float scale;
    int skip;
    long long steps, clipped, skipped;
};
constexpr int kSumsqParts = 512;  // workgroups (= partial sums) per run of k_sumsq
struct SumsqArgs {
    const float *g[9];
    int64_t n[9];
    int slot[9];
    int count;   // runs in this launch (<= 9), each into its own slot
};
// ctl->slot[a.slot[e]] = sum_i (double)g[e][i]^2 for every run e < a.count, in two stages: kSumsqParts workgroups per run own one fixed
// contiguous chunk each (thread t of a workgroup adds the 4-element groups t, t + 256, ... of the chunk in that order, then a fixed
// tree), then one workgroup per run adds the partials in index order.  No atomics: the result is a function of the data and n alone.
// parts: [9][kSumsqParts] doubles, slice a.slot[e] is run e's.
void k_sumsq(hipStream_t st, const SumsqArgs &a, double *parts, ClipCtl *ctl);
// norm = sqrt(slot[0] + ... + slot[n_slots - 1]) (slot order, double); skip = !isfinite(norm);
// scale = (!skip && norm > max_norm) ? (float)(max_norm / norm) : 1; steps += 1, clipped += scale applies, skipped += skip.
void k_clip_set(hipStream_t st, ClipCtl *ctl, int n_slots, float max_norm);
// out[i] = a[i] * b[i]
void k_mul_f32(hipStream_t st, const float *a, const float *b, int64_t n, float *out);

// ---- decode_kernels.hip: beam search (lrcn.jl:644-678) and the batched decode step (decode.hip) ----
// batched beam search: histories = [bos, 0, ...], next input = bos, probabilities = 1 for all R hypotheses (lrcn.jl:608-611)
void k_beam_init(hipStream_t st, int32_t *seq, int32_t *last, float *p, int R, int Lh, int bos);
// One decode step of beam bookkeeping for N images (one workgroup each): see beam_update_kernel.  K <= 32.
void k_beam_update(hipStream_t st, const int32_t *topi, const float *topv, const int32_t *seq_in, int32_t *seq_out, float *p,
                   int32_t *parent, int32_t *last, int32_t *done, int32_t *ndone, int32_t *res_tok, int32_t *res_len, float *res_p, int N,
                   int K, int L, int current, int nword, int eos);
// For each of R rows of prob [R][ld]: the K largest entries in descending order, ties to the lower index.
void k_topk_rows(hipStream_t st, const float *prob, int64_t ld, int R, int V, int K, int32_t *idx, float *val);
// prob[v] = exp(logp) for one row each (beam search, lrcn.jl:652).
void k_softmax_rows(hipStream_t st, const float *logits, int64_t ld_l, int M, int V, float *prob, int64_t ld_p);
// out[v] = (x[v] - max) - log(sum exp(x - max)) for one row each (the n-best beam above k_softmax_topk_rows' V limit)
void k_log_softmax_rows(hipStream_t st, const float *logits, int64_t ld_l, int M, int V, float *out, int64_t ld_o);
// softmax + top-K of every row in one pass (false: V too large for the register-resident form, use the two kernels)
// logp: log-probabilities (x - max) - log(sum exp(x - max)) instead of probabilities (the n-best beam), same order
bool k_softmax_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, int32_t *idx, float *val, bool logp = false);
// second half of the logits GEMM's softmax / top-K epilogue (gemm.h SmaxEpi): records [R][nrec][SMAX_REC] -> idx / val [R][K] as k_softmax_topk_rows;
// false = not applicable (K >= SMAX_KC, too many records)
bool k_softmax_topk_merge(hipStream_t st, const float *part, int nrec, int R, int K, int32_t *idx, float *val, bool logp = false);
// out[i][r][:] = in[i][parent[r]][:] for the four recurrent states (row stride C[i]); hT[i] != NULL also receives a T copy (ld ldT[i])
void k_gather_state(hipStream_t st, int dtype, const float *const in[4], float *const out[4], void *const hT[4], const int64_t ldT[4],
                    const int C[4], const int32_t *parent, int R);
// bf16 batched decode, one launch per step: embedding of each hypothesis' last token + h1 / h2 of its parent into the [x | h] operands
void k_decode_prep(hipStream_t st, const void *wembT, int64_t ld_w, const int32_t *last, const int32_t *parent, int R, int E, const void *h1,
                   int64_t ld_h1, int H1, const void *h2, int64_t ld_h2, int H2, void *xh1, int64_t ld_xh1, int64_t off_h1, void *xh2, int64_t ld_xh2,
                   int64_t off_h2);
// decode step with input-projection tables: the parents' bf16 h into the gate GEMMs' operands; out[r] = r / K (the image of a hypothesis row)
void k_decode_prep_h(hipStream_t st, const int32_t *parent, int R, const void *h1, int64_t ld_h1, int H1, const void *h2, int64_t ld_h2, int H2,
                     void *a1, int64_t ld_a1, void *a2, int64_t ld_a2, int64_t off_h2);
void k_row_div(hipStream_t st, int32_t *out, int R, int K);
// out[r][0..C) = in[r / K][0..C): every image row repeated K times (rows ld apart in both)
void k_repeat_rows(hipStream_t st, int dtype, const void *in, int64_t ld, int N, int K, int C, void *out);
// out[r][0..C) = in[src_row[r]][0..C)  (beam search parent-state gather, lrcn.jl:673-676); in != out.
void k_gather_rows_f32(hipStream_t st, const float *in, int64_t ld, const int32_t *src_row, int R, int C, float *out);

// ---- constrain.hip: the constrained top-K of a decode step (include/lrcn_constrain.h) ----
// What is not allowed at step `current` (1-based) for row r, whose history (bos first) is hist[r * ld_hist + 0 .. current - 1]: the columns
// of the static bitmap ban [(V + 31) / 32] (NULL: none; bits past V are zero), eos while current <= min_len, and with ngram = n >= 1 every
// word that would complete an n-gram the history already holds.  current <= 257.
struct ConstrainArgs {
    const uint32_t *ban;
    const int32_t *hist;
    int64_t ld_hist;
    int current, min_len, ngram, eos;
};
// For each of R rows of f32 logits [R][ld]: the K best allowed columns by logp = (z - max z) - log(sum exp(z - max z)) over ALL V columns,
// descending, ties to the lower column -- k_softmax_topk_rows' LOGP form (the same normaliser, bit for bit) on the allowed columns.
// false: V too large for the register-resident form; then k_log_softmax_rows, k_constrain_mask_rows on its output and k_topk_rows.
bool k_constrained_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, const ConstrainArgs &a, int32_t *idx,
                             float *val);
// lp[r][v] = -inf for every column v that is not allowed for row r (any V)
void k_constrain_mask_rows(hipStream_t st, float *lp, int64_t ld, int R, int V, const ConstrainArgs &a);

// ---- ensemble.hip: the mixture row of an ensemble decode step (include/lrcn_ensemble.h) ----
// The M members' f32 logits z[m] [R][ld[m]] and normalised weights, by value: no pointer table is uploaded.  Entries from M on are not read.
constexpr int kEnsembleMax = 8;   // LRCN_ENSEMBLE_MAX
struct EnsembleMixArgs {
    const float *z[kEnsembleMax];
    int64_t ld[kEnsembleMax];
    float w[kEnsembleMax];
    int M;
};
// out[r][v] = the mixture of the members' log-softmax rows (log_mean: the weighted sum of the log-probabilities, else the log of the
// weighted sum of the probabilities), any R >= 1, V >= 1, ld >= V and alignment; `out` overlaps no input.  One workgroup per row, no atomics.
void k_ensemble_mix_rows(hipStream_t st, const EnsembleMixArgs &a, bool log_mean, int R, int V, float *out, int64_t ld_out);

// ---- image_kernels.hip: the VGG side (vgg.hip, conv64.hip, conv64f.hip) ----
// conv weight (3,3,Cin,Cout) column-major f32 -> [Cout][tap = b*3+a][Cin_pad] T (zero padded channels)
void k_repack_conv_w(hipStream_t st, int dtype, const float *w, int Cin, int Cout, int Cin_pad, void *out);
// conv1_1 weight -> [64][ld] T with k = tap*3 + c (27 real, rest zero)
void k_repack_conv11_w(hipStream_t st, int dtype, const float *w, int Cout, void *out, int64_t ld);
// out = (bf16)(img - mean[c]) over n = N*S*S*3 bytes, written INSIDE A FRAME of 2 zero pixels: out[n][S+4][S+4][3], pixel (x, y) of the crop at
// [x+2][y+2]; the frame is never written (the buffer is zero since allocation) -- the input of conv64 FUSE, whose raw-window DMA reads
// conv1_1's zero padding from it.  Needs (N*(S+4)*(S+4)*3 + 8) elements.
// avg != NULL: subtract the full averageImage (S,S,3) column-major, avg(col, row, c) from pixel (row, col, c) (lrcn.jl:770-771), instead
void k_img_u8_to_bf16(hipStream_t st, const uint8_t *img, int64_t n, float m0, float m1, float m2, const float *avg, int S, void *out);
// batched resize + centre crop + grey -> RGB of variable-size decoded uint8 images (lrcn.jl:755-765): meta = device array of
// {int64 byte offset into src, int h, w, channels, pad} per image; out = uint8 crops [N][S][S][3]
void k_resize_crop_u8(hipStream_t st, const uint8_t *src, const void *meta, int N, int S, uint8_t *out);
// feats (N x F column-major f32): every row divided by its sum (lrcn.jl:595-597)
void k_normalize_rows(hipStream_t st, float *feats, int N, int F);
// conv1_1 weight -> [64][32] bf16 in the K order of the fused conv1_1+conv1_2 kernel (conv64.hip, FUSE)
void k_repack_conv11_w_fused(hipStream_t st, const float *w, const float *b, void *out);  // b: conv1_1 bias (pieces at k' = 27..29), may be NULL
// fc6 weight (4096 x 25088 column-major, k_ref = x + 7y + 49c) -> [4096][25088] T with k = (y*7+x)*512 + c
void k_repack_fc6_w(hipStream_t st, int dtype, const float *w, void *out);
// conv1_1 im2col from uint8 crops img[n][row][col][3]: A[m][k = tap*3+c] (T, ld), m window-major over (y=col, x=row);
// value = pixel - mean[c], zero outside the image.                               (lrcn.jl:766-772 + :724)
void k_im2col11_u8(hipStream_t st, int dtype, const uint8_t *img, int N, int S, float m0, float m1, float m2, void *out,
                   int64_t ld);
// same from the preprocessed float tensor x (S,S,3,N) column-major
void k_im2col11_f32(hipStream_t st, int dtype, const float *x, int N, int S, void *out, int64_t ld);
// out(i,j,c,n) = img[n][i][j][c] - mean[c]   (lrcn.jl:766-772)
void k_preprocess_u8(hipStream_t st, const uint8_t *img, int N, int S, float m0, float m1, float m2, const float *avg, float *out);
// reference (W,H,C,N) column-major f32 <-> internal NHWC [n][y][x][C_ld] T   (x = dim 1, y = dim 2)
void k_ref_to_nhwc(hipStream_t st, int dtype, const float *x, int W, int H, int C, int N, void *out, int C_ld);
void k_nhwc_to_ref(hipStream_t st, int dtype, const void *in, int W, int H, int C, int N, int C_ld, float *out);

// ---- sample.hip: the per-step draw of the sampled decode (lrcn_sample_batch) ----
// Device state of R independent rows: histories seq [R][L] (bos first), next input last[R], log-likelihood logp[R], done[R] / len[R],
// ndone = number of finished rows.  A row stops after eos or at current > nword.
struct SampleState {
    int32_t *seq, *last, *done, *len, *ndone;
    float *logp;
    int L, current, nword, eos;
};
void k_sample_init(hipStream_t st, const SampleState &s, int R, int bos);
// from f32 logits [R][ld]: one workgroup per row (any V; top_k 0 = all columns, else <= 32; temp 0 = greedy)
void k_sample_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int top_k, float temp, uint64_t seed, int S, const SampleState &s);
// from GEMM_OUT_SMAX_GUMBEL records (top_k = 0) resp. GEMM_OUT_SMAX_TOPK records (1 <= top_k < SMAX_KC); false = not applicable
bool k_sample_gumbel_merge(hipStream_t st, const float *part, int nrec, int R, const SampleState &s);
bool k_sample_topk_merge(hipStream_t st, const float *part, int nrec, int R, int top_k, float temp, uint64_t seed, int S, const SampleState &s);
// the selection of include/lrcn_nucleus.h (any top_k <= V, top_p in (0, 1]) and the draw, from f32 logits [R][ld], one workgroup per row, any
// V >= 1.  s given: step s->current of the batched decode (commits to the state, skips finished rows); s NULL: step `current` into
// out_tok / out_logp [R] (out_logp may be NULL).  count (may be NULL): row r's admitted-set size to count[r * count_ld].
void k_sample_nucleus(hipStream_t st, const float *logits, int64_t ld, int R, int V, int S, int current, float temp, int top_k, float top_p,
                      uint64_t seed, const SampleState *s, int32_t *count, int64_t count_ld, int32_t *out_tok, float *out_logp);

// ---- score.hip: the per-pair steps of caption scoring (lrcn_score_matrix / lrcn_score_pairs) ----
// A2 (T) row r < R: columns [0, h) = P row row_cap[r] (P: this step's [caption][ldP] block of h1 Wproj), columns [h2_off, h2_off + zero_h2) = 0
// (the first step's zero h2); tgt_row[r] = tgt_cap[row_cap[r]]
void k_score_prep(hipStream_t st, int dtype, void *A2, int64_t ldA2, const void *P, int64_t ldP, const int32_t *row_cap, int R, int h, int zero_h2,
                  int64_t h2_off, const int32_t *tgt_cap, int32_t *tgt_row);
// dst f32 [R][C] = table rows idx[r] (C % 4 == 0)
void k_score_gather_rows(hipStream_t st, const float *table, int C, const int32_t *idx, int R, float *dst);
// acc[r] += z[tgt] - max - log(sum exp) from the row's GEMM_OUT_SMAX_PICK records; false = too many records
bool k_score_pick_merge(hipStream_t st, const float *part, int nrec, int R, double *acc);
void k_score_acc(hipStream_t st, const double *terms, int R, double *acc);                        // acc[r] += terms[r]
// rows r0 .. r0+R of the N x M matrix, caption-major over the sorted captions ord[]: image r % N, sorted caption r / N, slot n + ord[j] * N
void k_score_matrix_rows(hipStream_t st, int64_t r0, int R, int N, const int32_t *ord, int32_t *img, int32_t *cap, int32_t *out);
void k_score_scatter(hipStream_t st, const double *acc, const int32_t *out_idx, int R, float *scores);  // scores[out_idx[r]] = acc[r]

// ---- nbest.hip: the per-step bookkeeping of the n-best beam (lrcn_beam_nbest_batch, include/lrcn_nbest.h) ----
// Device state of N images x K slots (row r = n * K + k): live histories (ping-pong) and their cumulative log-probabilities (-inf: dead
// slot); per image {live slots (a prefix), pool entries, done}; the pool of finished hypotheses, [N][K] best first, each {score, logp (float
// bits), storage row, length}, whose tokens live in 2K storage rows per image (an entry never moves its tokens); the results, written when
// an image is done.
struct NbestState {
    const int32_t *seq_in;
    int32_t *seq_out, *parent, *last, *ndone;
    int4 *img;                                         // [N] {nlive, pool count, done, 0}
    float *cum;
    int32_t *store;                                    // [N][2K][L]
    int4 *pool;                                        // [N][K]
    int32_t *res_tok, *res_len;                        // [N*K][L], [N*K]
    float *res_logp, *res_score;                       // [N*K]
    int K, L, current, nword, eos;
    float lp_cur, lp_max;                              // (float)pow(current, alpha), (float)pow(nword + 1, alpha)
};
// every slot [bos], cum 0, one live slot, empty pool, not done (R = N * K rows)
void k_nbest_init(hipStream_t st, const NbestState &s, int N, int bos);
// one step for N images (one workgroup each) from this step's log-probability top-K topi / topv [N*K][K]; K <= 32
void k_nbest_update(hipStream_t st, const int32_t *topi, const float *topv, const NbestState &s, int N);

// ---- diverse.hip: the per-step bookkeeping of diverse beam search (lrcn_beam_diverse_batch, include/lrcn_diverse.h) ----
// The n-best state with K = the full width, read as G groups of K' = K / G per image: group g of image n owns rows n*K + g*K' .. + K'-1 of
// the histories, cum and the results, entries g*K' .. of the image's pool and storage rows g*2K' .. of its 2K; img is [N*G] group records
// {live slots, pool entries, dead, satisfied}; done [N] marks the images whose results are written.
struct DiverseState {
    NbestState nb;
    int32_t *done;
    int G;
    float lambda;
};
void k_diverse_init(hipStream_t st, const DiverseState &s, int N, int bos);
// one step for N images (one workgroup each) from this step's log-probability top-K topi / topv [N*K][K] (the full width); K <= 32
void k_diverse_update(hipStream_t st, const int32_t *topi, const float *topv, const DiverseState &s, int N);

// ---- forced words (include/lrcn_forced.h): the top-K of a row that knows its state (constrain.hip), the bank bookkeeping (forced.hip) ----
constexpr int kForcedMaxSets = 3, kForcedMaxAlt = 4, kForcedMaxWords = kForcedMaxSets * kForcedMaxAlt;
// The word table words [images][C*A] on the device (-1: no word); row r belongs to image r / rows_per_image.
struct ForcedArgs {
    const int32_t *words;
    int C, A, rows_per_image;
};
// k_constrained_topk_rows with the forced-word rules: idx / val [R][K] the row's K best STAY columns (allowed by rules 1-4 and no word of a
// present, unsatisfied set of the row), move [R][C*A] the logp of the row's move words (-inf: absent, satisfied set, or banned by rules
// 1-3), state [R] the sets the row's history has met.  false: V too large for the register-resident form; then k_log_softmax_rows,
// k_forced_mask_rows on its output and k_topk_rows.
bool k_forced_topk_rows(hipStream_t st, const float *logits, int64_t ld, int R, int V, int K, const ConstrainArgs &a, const ForcedArgs &f,
                        int32_t *idx, float *val, float *move, int32_t *state);
// the general form's middle step, any V: lp [R][ld] is the rows' log-softmax; gathers move and state as above, then writes -inf over every
// column that is no stay column
void k_forced_mask_rows(hipStream_t st, float *lp, int64_t ld, int R, int V, const ConstrainArgs &a, const ForcedArgs &f, float *move,
                        int32_t *state);
// The n-best state with nb.K = the width of ONE bank: image n owns S * K rows (S = 2^C banks of K), bank b rows n*S*K + b*K ..; cum,
// histories, parent and last are per row; img is [N*S] bank records {live slots (a prefix), -, -, -} with the image's pool count in bank
// 0's .y; the pool, its 2K storage rows and the results use the first K rows of each image; done [N] marks the images whose results are
// written.  move [N*S*K][C*A]: this step's move values from k_forced_topk_rows.
struct ForcedState {
    NbestState nb;
    int32_t *done;
    const int32_t *words;
    const float *move;
    int C, A;
};
void k_forced_init(hipStream_t st, const ForcedState &s, int N, int bos);
// one step for N images (one workgroup each) from this step's stay proposals topi / topv [N*S*K][K] and s.move; S * K <= 32
void k_forced_update(hipStream_t st, const int32_t *topi, const float *topv, const ForcedState &s, int N);
