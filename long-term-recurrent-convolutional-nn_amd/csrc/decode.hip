// decode.hip -- the caption model's decoding (include/lrcn.h, lrcn_sample.h, lrcn_nucleus.h, lrcn_nbest.h, lrcn_diverse.h, lrcn_constrain.h, lrcn_ensemble.h, lrcn_forced.h, lrcn_score.h): the batched decode's routes,
// tables, begin and step, and on top of them the single-image and batched beam search, sampling, the n-best and diverse beams (and their
// constrained form, lrcn_constrain.h, their ensemble form, lrcn_ensemble.h, and the forced-word form, lrcn_forced.h) and caption scoring;
// the step's test entry (lrcn_decode_debug.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/lrcn_constrain.h"
#include "../../include/lrcn_ensemble.h"
#include "../../include/lrcn_forced.h"
#include "../../include/lrcn_decode_debug.h"
#include "../../include/lrcn_nbest.h"
#include "../../include/lrcn_diverse.h"
#include "../../include/lrcn_nucleus.h"
#include "../../include/lrcn_sample.h"
#include "../../include/lrcn_score.h"
#include "ctx.h"

using namespace lrcn_impl;

namespace {

// The batched decode (lrcn_beam_search_batch, lrcn_sample_batch) runs the same step on the concatenated buffers: st_xh1 = [x | h1],
// st_xh2 = [x2 | h2] (T, the h blocks already hold this step's input states), one GEMM per LSTM against W1cat / W2cat.  LRCN-1f:
// st_xh1 = [emb | x_cnn | h1] (decode_begin writes the x_cnn columns once: they do not change during a decode).  Its routes below
// (decode_route) are chosen once per call; decode_begin and decode_step drive them.
// The batched decode step with the cell math in the gate GEMM's epilogue (gemm_8p.hip GEMM_OUT_LSTM_FWD; round 5): from 256 hypotheses
// the gate GEMM is a chip-filling contraction (5120 x 4000 x 2048 at 1024 images x 5 beams), and the f32 pre-activations it used to write
// for a separate cell kernel -- 82 MB out and back per layer and step, plus the kernel -- never leave the workgroup.  The concatenated
// weights are then made with (unit, gate)-interleaved rows (prepare_weights cat_perm), the bias rides in as a broadcast row, the
// activated gates are not kept (no backward pass).  LRCN_DECODE_EPI=0: GEMM + cell kernel as before.
bool decode_epi_on(const lrcn_ctx *c, int B) {
    return !knob_off("LRCN_DECODE_EPI") && c->dt == GEMM_T_BF16 && B >= 256 && !(c->H1 & 3) && !(c->H2 & 3);
}
int decode_gates_epi(lrcn_ctx *c, const void *xh, int64_t ldxh, const void *Wcat, int K, const float *bias, int B, int H, const float *c_prev,
                     const int32_t *c_prev_idx, float *c_out, void *h_out, int64_t ld_h_out, const int32_t *gx_idx = nullptr) {
    // bias: ONE row [4H] for every row, or -- gx_idx given -- a table of input-side pre-activations of which row r adds row gx_idx[r]
    // h_out must NOT be the h columns of `xh`: every tile of this launch reads them as A-operand columns, and tiles of one row block run in
    // different rounds (2.5 rounds of 256 x 128 tiles at 5120 x 4000), so an in-place h(t) would reach tiles that still need h(t-1).
    GemmArgs g{};
    g.dtype = c->dt;
    g.A = xh; g.lda = ldxh;
    g.B = Wcat; g.ldb = ldxh;
    g.M = B; g.N = 4 * H;
    g.K = (int)round_up64(K, 64);  // whole 128-byte K-steps: both operands carry zeros in the padding (as gemm() does)
    if (g.K > ldxh) FAIL(c, LRCN_EINVAL, "decode step: K = %d exceeds the operand rows (%lld)", g.K, (long long)ldxh);
    g.a_mode = GEMM_A_PLAIN;
    g.out_mode = GEMM_OUT_LSTM_FWD;
    g.zero_page = c->zero_page;
    g.lstm.H = H; g.lstm.ld_a = 4 * H; g.lstm.ld_h = ld_h_out;
    g.lstm.Gx = bias; g.lstm.gx_bcast = gx_idx ? 0 : 1; g.lstm.gx_idx = gx_idx;
    // the cell state of row r continues its PARENT hypothesis' (lrcn.jl:673-676): read through c_prev_idx (round 6; NULL = the first step,
    // zero state) into the other buffer of the pair -- no gather launch between the steps
    g.lstm.c_prev = c_prev; g.lstm.c_prev_idx = c_prev_idx; g.lstm.c_out = c_out;
    g.lstm.acts = nullptr;
    g.lstm.h_new = h_out;
    g.lstm.h_f32 = nullptr;
    hipError_t e = launch_gemm_8p(c->stream, g);
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "decode step (gate GEMM + cell epilogue): %s", hipGetErrorString(e));
    return LRCN_OK;
}

// The logits GEMM of a batched decode step with softmax + top-K in its epilogue (gemm_8p.hip GEMM_OUT_SMAX_TOPK; round 6): x * w[end-1] .+ w[end]
// (lrcn.jl:550) is reduced tile by tile to per-row records and merged by k_softmax_topk_merge -- the B x V f32 logits (218 MB per step at
// 5120 x 10640) are never written, and softmax_topk_rows_kernel's pass over them disappears.  LRCN_DECODE_SMAX=0: GEMM + that kernel.
int smax_nrec(const lrcn_ctx *c) { return 2 * ((c->V + 255) / 256); }
// Where a logits GEMM of R rows may reduce to records at all (every record route -- the decode's and the scoring's -- asks here): bf16,
// from 256 rows, V % 4 == 0, >= 2 K-tiles, and no more records per row than the merges hold (V <= 32768).  Elsewhere the f32 logits route.
bool smax_records_on(const lrcn_ctx *c, int R) {
    return c->dt == GEMM_T_BF16 && R >= 256 && c->V >= 256 && !(c->V & 3) && c->H2 > 64 && smax_nrec(c) <= SMAX_MAX_NREC;
}
bool decode_smax_on(const lrcn_ctx *c, int B, int K) {
    return !knob_off("LRCN_DECODE_SMAX") && K < SMAX_KC && smax_records_on(c, B);
}
// The same logits GEMM with any of the record epilogues (GEMM_OUT_SMAX_TOPK / _GUMBEL / _PICK) for M rows of h: every 128 columns of a row
// reduce to one record of smax_part [M][smax_nrec][SMAX_REC] (allocated on first use, max_B rows).  e: the out-mode's own SmaxEpi fields
// (GUMBEL: the draw parameters, PICK: the target columns); part and nrec are filled in here.
int logits_records(lrcn_ctx *c, const void *hT, int64_t ldh, const float *bias, int M, int out_mode, const SmaxEpi &e) {
    const int nrec = smax_nrec(c);
    if (!c->smax_part) DALLOC(c, c->smax_part, sizeof(float) * (size_t)c->maxB * nrec * SMAX_REC);
    GemmArgs g{};
    g.dtype = c->dt;
    g.A = hT; g.lda = ldh;
    g.B = c->Wod; g.ldb = c->ldH2;
    g.M = M; g.N = c->V;
    g.K = (int)round_up64(c->H2, 64);
    if (g.K > ldh || g.K > c->ldH2) FAIL(c, LRCN_EINVAL, "logits GEMM: K = %d exceeds the operand rows", g.K);
    g.bias = bias;
    g.a_mode = GEMM_A_PLAIN;
    g.out_mode = out_mode;
    g.zero_page = c->zero_page;
    g.smax = e;
    g.smax.part = c->smax_part; g.smax.nrec = nrec;
    hipError_t err = launch_gemm_8p(c->stream, g);
    if (err != hipSuccess) FAIL(c, LRCN_EHIP, "logits GEMM + softmax records epilogue (out_mode %d): %s", out_mode, hipGetErrorString(err));
    return LRCN_OK;
}

// Where the logits of a batched decode step go, fixed by the caller for the whole call:
//   LOGITS   f32 logits in st_logits [B][ldV] (every route without decode_smax_on)
//   TOPK     the K best columns of every row in st_topi / st_topv (the beams): GEMM_OUT_SMAX_TOPK records merged where the route has them
//            (`records`: DecodeRoute::smax), else the f32 logits and the softmax / top-K rows kernels
//   RECORDS  GEMM_OUT_SMAX_TOPK records only, left in smax_part (the sampler at top_k >= 1 merges them itself)
//   GUMBEL   GEMM_OUT_SMAX_GUMBEL records, left in smax_part, with the draw parameters `draw` (the sampler at top_k = 0, which sets
//            draw.current before every step)
//   logp     with TOPK: log-probabilities instead of probabilities in st_topv (the n-best beam)
struct DecodeTail {
    enum Kind { LOGITS, TOPK, RECORDS, GUMBEL } kind = LOGITS;
    int K = 0;
    bool logp = false;
    bool records = false;
    SmaxEpi draw{};
};
// :652, :655-656 on the f32 logits in st_logits: the top K (log-)probabilities of each of R rows into st_topi / st_topv, in one pass where
// the rows kernel fits, else the (log-)softmax of every row into st_prob and then its top K
void topk_rows(lrcn_ctx *c, int R, int K, bool logp) {
    if (k_softmax_topk_rows(c->stream, c->st_logits, c->ldV, R, c->V, K, c->st_topi, c->st_topv, logp)) return;
    if (logp)
        k_log_softmax_rows(c->stream, c->st_logits, c->ldV, R, c->V, c->st_prob, c->ldV);
    else
        k_softmax_rows(c->stream, c->st_logits, c->ldV, R, c->V, c->st_prob, c->ldV);
    k_topk_rows(c->stream, c->st_prob, c->ldV, R, c->V, K, c->st_topi, c->st_topv);
}
int decode_logits(lrcn_ctx *c, const float *const p[9], const void *hT, int64_t ldh, int B, const DecodeTail &t) {
    if (t.kind == DecodeTail::LOGITS || (t.kind == DecodeTail::TOPK && !t.records)) {
        GEMM(c, c->dt, hT, ldh, c->Wod, c->ldH2, c->st_logits, c->ldV, B, c->V, c->H2, p[8], true);   // lrcn.jl:550
        if (t.kind == DecodeTail::TOPK) topk_rows(c, B, t.K, t.logp);
        return LRCN_OK;
    }
    int r = logits_records(c, hT, ldh, p[8], B, t.kind == DecodeTail::GUMBEL ? GEMM_OUT_SMAX_GUMBEL : GEMM_OUT_SMAX_TOPK, t.draw);
    if (r || t.kind != DecodeTail::TOPK) return r;
    if (!k_softmax_topk_merge(c->stream, c->smax_part, smax_nrec(c), B, t.K, c->st_topi, c->st_topv, t.logp))
        FAIL(c, LRCN_EINVAL, "softmax / top-K merge: K = %d, %d records", t.K, smax_nrec(c));
    return LRCN_OK;
}

// The batched decode step with input-projection TABLES (round 6).  [x | h] W of lrcn.jl:529 is x Wx + h Wh, and in a decode x is not free:
// LSTM-1's x is the embedding of one of V tokens, LSTM-2's is [h1 Wproj | x_cnn] with x_cnn fixed per image (lrcn.jl:546, :611).  So
// T1 = Wembed W1x + b1 (V x 4H1: 85 GFLOP once per call -- what ONE step spent on it for its 5120 rows) and U2 = x_cnn W2x[right half] + b2
// (one row per image) are made once, each step's gate GEMMs contract h (K = 1024) resp. [h1 Wproj | h2] (K = 1536) instead of 2048, and the
// cell epilogue adds row last_token / row image of the tables (LstmEpi::gx_idx).  63 of a step's 282 GFLOP at 5120 hypotheses are not done,
// the embedding gather and the concat launch disappear.  Same products, f32 accumulation in two chains instead of one.  Memory for FLOPs:
// T1 is 170 MB of the 288 GB.  LRCN_DECODE_TABLES=0: the [x | h] form.
bool decode_tables_on(const lrcn_ctx *c, int B) {
    return !knob_off("LRCN_DECODE_TABLES") && c->nl == 2 && decode_epi_on(c, B) && c->H1 > 64 && c->H2 > 64;
}
int decode_tables_alloc(lrcn_ctx *c) {
    const size_t es = c->esz;
    if (!c->dec_T1) DALLOC(c, c->dec_T1, sizeof(float) * (size_t)c->V * 4 * c->H1);
    if (!c->dec_U2) DALLOC(c, c->dec_U2, sizeof(float) * (size_t)c->maxB * 4 * c->H2);
    if (!c->dec_A1) DALLOC(c, c->dec_A1, es * (size_t)c->maxB * c->ldH1);
    if (!c->dec_A2) DALLOC(c, c->dec_A2, es * (size_t)c->maxB * (c->ldh + c->ldH2));
    if (!c->dec_W2c) DALLOC(c, c->dec_W2c, es * (size_t)4 * c->H2 * (c->ldh + c->ldH2));
    if (!c->dec_Aimg) DALLOC(c, c->dec_Aimg, es * (size_t)c->maxB * c->ldH2);
    if (!c->dec_img) DALLOC(c, c->dec_img, sizeof(int32_t) * (size_t)c->maxB);
    return LRCN_OK;
}
// once per decode call, after prepare_weights(dec_tables) and the image embedding (dxcnn [N][ldh] f32): the two tables and the row -> image map
int decode_tables_build(lrcn_ctx *c, const float *const p[9], int N, int K) {
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V;
    hipStream_t st = c->stream;
    GEMM(c, dt, c->WeT, c->ldE, c->W1x, c->ldX1, c->dec_T1, 4 * H1, V, 4 * H1, E, p[1], true);                 // per token
    HIPCHK(c, hipMemsetAsync(c->dec_Aimg, 0, c->esz * (size_t)N * c->ldH2, st));
    DropSpec none{};
    k_concat_x2(st, dt, c->dec_Aimg, c->ldH2, c->dxcnn, c->ldh, 1, N, h, h, none);                              // [0 | x_cnn] per image
    GEMM(c, dt, c->dec_Aimg, c->ldH2, c->W2x, c->ldH2, c->dec_U2, 4 * H2, N, 4 * H2, H2, p[3], true);           // per image
    k_row_div(st, c->dec_img, N * K, K);
    HIPCHK(c, hipMemsetAsync(c->dec_A1, 0, c->esz * (size_t)N * K * c->ldH1, st));                              // zero initial h1 / h2 and K padding
    HIPCHK(c, hipMemsetAsync(c->dec_A2, 0, c->esz * (size_t)N * K * (c->ldh + c->ldH2), st));
    KCHK(c, "decode tables");
    return LRCN_OK;
}

// The route of a batched decode of R rows, chosen once per call.  K_records: the top-K width its logits epilogue would keep (the beam's K,
// the sampler's top_k).
struct DecodeRoute {
    bool epi, smax, tables;
};
DecodeRoute decode_route(const lrcn_ctx *c, int R, int K_records) {
    const bool epi = decode_epi_on(c, R);
    return DecodeRoute{epi, epi && decode_smax_on(c, R, K_records), epi && decode_tables_on(c, R)};
}

// Everything a batched decode of N images x per_image rows (row r belongs to image r / per_image) does before its first step: the route's
// weight copies, input = input * param[end-3] per image (lrcn.jl:611) repeated for the image's rows, zero states and [x | h] operands (their
// K padding included), LRCN-1f's x_cnn columns of [emb | x_cnn | h1] (constant over the decode: a row never changes image), the tables.
// The caller's own bookkeeping (histories, done flags, st_parent) follows it.
int decode_begin(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int per_image, const DecodeRoute &rt) {
    const int dt = c->dt, H1 = c->H1, H2 = c->H2, h = c->h, R = N * per_image;
    hipStream_t st = c->stream;
    int r = rt.tables ? decode_tables_alloc(c) : LRCN_OK;
    ShadowNeed sh{};
    sh.cat = !rt.tables; sh.cat_perm = rt.epi; sh.dec_tables = rt.tables;
    if (r || (r = prepare_weights(c, p, sh))) return r;
    k_transpose(st, dt, 1, feats, N, LRCN_CNNOUT, N, c->F, LRCN_CNNOUT, 0);
    GEMM(c, dt, c->F, LRCN_CNNOUT, c->Wcd, LRCN_CNNOUT, c->dxcnn, c->ldh, N, h, LRCN_CNNOUT, nullptr, true);
    k_repeat_rows(st, GEMM_T_F32, c->dxcnn, c->ldh, N, per_image, h, c->xcnn);
    const int Hs[4] = {H1, H1, H2, H2};
    for (int i = 0; i < 4; ++i) HIPCHK(c, hipMemsetAsync(c->st_f32[i], 0, sizeof(float) * (size_t)R * Hs[i], st));
    HIPCHK(c, hipMemsetAsync(c->st_xh1, 0, c->esz * (size_t)R * c->ldXH1, st));  // zero initial h1 / h2 (T copies) and K padding
    HIPCHK(c, hipMemsetAsync(c->st_xh2, 0, c->esz * (size_t)R * c->ldXH2, st));
    if (c->nl == 1) {
        DropSpec none{};
        k_concat_x2(st, dt, c->st_xh1, c->ldXH1, c->xcnn, c->ldh, 1, R, c->E, h, none);
    }
    return rt.tables ? decode_tables_build(c, p, N, per_image) : LRCN_OK;
}

// The three forms of a batched decode step (lrcn.jl:650-651 for all B rows at once): the input token of row r is bs_last[r]; its states
// continue row parent[r]'s (parent NULL: the first step, zero states).  Each ends in decode_logits.
// Tables (decode_tables_on): the parents' h1 / h2 into the gate GEMMs' operands, the cell epilogues add the token's / image's table row.
int step_tables(lrcn_ctx *c, const float *const p[9], int B, const int32_t *parent, const DecodeTail &tail) {
    const int dt = c->dt, H1 = c->H1, H2 = c->H2, h = c->h;
    const int64_t ldA2 = c->ldh + c->ldH2;
    if (parent) k_decode_prep_h(c->stream, parent, B, c->st_h1, c->ldH1, H1, c->st_h2, c->ldH2, H2, c->dec_A1, c->ldH1, c->dec_A2, ldA2, c->ldh);
    int r = decode_gates_epi(c, c->dec_A1, c->ldH1, c->W1h_gi, H1, c->dec_T1, B, H1, parent ? c->st_f32[1] : nullptr, parent, c->st2_f32[1], c->st_h1,
                             c->ldH1, c->bs_last);
    if (r) return r;
    GEMM(c, dt, c->st_h1, c->ldH1, c->Wpd, c->ldH1, c->dec_A2, ldA2, B, h, H1, nullptr, false);   // x = s[1] * w[end-4] (lrcn.jl:544) into A2's left block
    r = decode_gates_epi(c, c->dec_A2, ldA2, c->dec_W2c, (int)ldA2, c->dec_U2, B, H2, parent ? c->st_f32[3] : nullptr, parent, c->st2_f32[3], c->st_h2,
                         c->ldH2, c->dec_img);
    if (r || (r = decode_logits(c, p, c->st_h2, c->ldH2, B, tail))) return r;
    KCHK(c, "decode step (tables)");
    return LRCN_OK;
}
// Cell epilogue (decode_epi_on): one launch writes the embedding of every row's token and its parent's h1 / h2 into the [x | h] operands; the
// epilogues write h(t) to st_h1 / st_h2 (never into the operand they are still reading) and c(t) to st2_f32[1] / [3].
int step_epi(lrcn_ctx *c, const float *const p[9], int B, const int32_t *parent, const DecodeTail &tail) {
    const int dt = c->dt, H1 = c->H1, H2 = c->H2, h = c->h;
    const bool two = c->nl == 2;
    hipStream_t st = c->stream;
    k_decode_prep(st, c->WeT, c->ldE, c->bs_last, parent, B, c->E, c->st_h1, c->ldH1, H1, two ? c->st_h2 : nullptr, c->ldH2, H2, c->st_xh1, c->ldXH1,
                  c->ldX1, two ? c->st_xh2 : nullptr, c->ldXH2, c->ldH2);
    int r = decode_gates_epi(c, c->st_xh1, c->ldXH1, c->W1cat, (int)c->ldX1 + H1, p[1], B, H1, parent ? c->st_f32[1] : nullptr, parent, c->st2_f32[1],
                             c->st_h1, c->ldH1);
    if (r) return r;
    if (two) {
        GEMM(c, dt, c->st_h1, c->ldH1, c->Wpd, c->ldH1, c->st_xh2, c->ldXH2, B, h, H1, nullptr, false);
        DropSpec none{};
        k_concat_x2(st, dt, c->st_xh2, c->ldXH2, c->xcnn, c->ldh, 1, B, h, h, none);
        r = decode_gates_epi(c, c->st_xh2, c->ldXH2, c->W2cat, (int)c->ldH2 + H2, p[3], B, H2, parent ? c->st_f32[3] : nullptr, parent, c->st2_f32[3],
                             c->st_h2, c->ldH2);
        if (r) return r;
    }
    if ((r = decode_logits(c, p, two ? c->st_h2 : c->st_h1, two ? c->ldH2 : c->ldH1, B, tail))) return r;
    KCHK(c, "decode step (cell epilogue)");
    return LRCN_OK;
}
// Plain: GEMM + cell kernel, the states updated in place (in st_f32 and the h blocks of st_xh1 / st_xh2).  It reads no parent: the caller
// moves the states to their rows' parents after the step where they differ.
int step_plain(lrcn_ctx *c, const float *const p[9], int B, const DecodeTail &tail) {
    const int dt = c->dt, H1 = c->H1, H2 = c->H2, h = c->h;
    hipStream_t st = c->stream;
    void *h1T = boff(c->st_xh1, c->ldX1, c->esz), *h2T = boff(c->st_xh2, c->ldH2, c->esz);
    DropSpec none{};
    k_embed_gather(st, dt, c->WeT, c->ldE, c->bs_last, 1, B, c->E, none, c->st_xh1, c->ldXH1);  // lrcn.jl:650
    GEMM(c, dt, c->st_xh1, c->ldXH1, c->W1cat, c->ldXH1, c->st_g, 4 * H1, B, 4 * H1, (int)c->ldX1 + H1, p[1], true);
    k_lstm_fwd(st, dt, c->st_g, 4 * H1, c->st_f32[1], B, H1, c->st_a, c->ld4H1, c->st_f32[1], h1T, c->ldXH1, c->st_f32[0]);
    if (c->nl == 2) {
        GEMM(c, dt, h1T, c->ldXH1, c->Wpd, c->ldH1, c->st_xh2, c->ldXH2, B, h, H1, nullptr, false);
        k_concat_x2(st, dt, c->st_xh2, c->ldXH2, c->xcnn, c->ldh, 1, B, h, h, none);
        GEMM(c, dt, c->st_xh2, c->ldXH2, c->W2cat, c->ldXH2, c->st_g, 4 * H2, B, 4 * H2, (int)c->ldH2 + H2, p[3], true);
        k_lstm_fwd(st, dt, c->st_g, 4 * H2, c->st_f32[3], B, H2, c->st_a, c->ld4H2, c->st_f32[3], h2T, c->ldXH2, c->st_f32[2]);
    }
    int r = c->nl == 2 ? decode_logits(c, p, h2T, c->ldXH2, B, tail) : decode_logits(c, p, h1T, c->ldXH1, B, tail);
    if (r) return r;
    KCHK(c, "decode step");
    return LRCN_OK;
}
// One step of a batched decode on the call's route; from the second step (current > 1) the tables and epilogue forms read the parents in
// st_parent.  The epilogue forms wrote c(t) into the other buffer of each pair: swapped here, so st_f32 holds every route's current states.
int decode_step(lrcn_ctx *c, const float *const p[9], int R, const DecodeRoute &rt, int current, const DecodeTail &tail) {
    const int32_t *parent = current > 1 ? c->st_parent : nullptr;
    int r = rt.tables ? step_tables(c, p, R, parent, tail) : rt.epi ? step_epi(c, p, R, parent, tail) : step_plain(c, p, R, tail);
    if (r || !rt.epi) return r;
    std::swap(c->st_f32[1], c->st2_f32[1]);
    if (c->nl == 2) std::swap(c->st_f32[3], c->st2_f32[3]);
    return LRCN_OK;
}
// After a beam step on the plain route, which read no parent: the four states of every row follow its parent in st_parent (lrcn.jl:673-676),
// and the T copies of h1 / h2 for the next step's GEMMs ride along.
void follow_parents(lrcn_ctx *c, int R) {
    const int Hs[4] = {c->H1, c->H1, c->H2, c->H2};
    void *const hT[4] = {boff(c->st_xh1, c->ldX1, c->esz), nullptr, boff(c->st_xh2, c->ldH2, c->esz), nullptr};
    const int64_t ldT[4] = {c->ldXH1, 0, c->ldXH2, 0};
    k_gather_state(c->stream, c->dt, c->st_f32, c->st2_f32, hT, ldT, Hs, c->st_parent, R);
    for (int i = 0; i < 4; ++i) std::swap(c->st_f32[i], c->st2_f32[i]);
}

// the context's pinned host staging buffer, grown to at least `need` bytes (decode results: see decode_results_to_host)
int pin_reserve(lrcn_ctx *c, size_t need) {
    if (need > c->pin_bytes) {
        if (c->pin) (void)hipHostFree(c->pin);
        c->pin = nullptr;
        c->pin_bytes = 0;
        if (hipHostMalloc(&c->pin, need, hipHostMallocDefault) != hipSuccess) FAIL(c, LRCN_ENOMEM, "hipHostMalloc(%zu) failed", need);
        c->pin_bytes = need;
    }
    return LRCN_OK;
}

// the early-exit test of a batched decode: have `target` images / rows finished (bs_ndone)?  One 4-byte read that waits for the stream.
int decode_poll_done(lrcn_ctx *c, int target, bool &done) {
    int32_t nd = 0;
    HIPCHK(c, hipMemcpyAsync(&nd, c->bs_ndone, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    done = nd >= target;
    return LRCN_OK;
}

// a batched decode's results -- tok [rows][Lh], len [rows], val [rows] (and val2 [rows] if given) on the device -- into the caller's host
// arrays (out_val, out_val2 may be NULL), through the context's PINNED staging buffer: a device -> pageable-host copy above 64 KB takes HIP's
// pin-on-the-fly path (measured: +16 ms per decode from 512 images, whose token block is 67 KB -- more than the 12.9 ms of kernels)
int decode_results_to_host(lrcn_ctx *c, const int32_t *tok, const int32_t *len, const float *val, int rows, int Lh, int32_t *out_tok, int *out_len,
                           float *out_val, const float *val2 = nullptr, float *out_val2 = nullptr) {
    const size_t nb_tok = sizeof(int32_t) * (size_t)rows * Lh, nb_n = sizeof(int32_t) * (size_t)rows;
    int r = pin_reserve(c, nb_tok + (val2 ? 3 : 2) * nb_n);
    if (r) return r;
    unsigned char *pin = reinterpret_cast<unsigned char *>(c->pin);
    HIPCHK(c, hipMemcpyAsync(pin, tok, nb_tok, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pin + nb_tok, len, nb_n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(pin + nb_tok + nb_n, val, nb_n, hipMemcpyDeviceToHost, c->stream));
    if (val2) HIPCHK(c, hipMemcpyAsync(pin + nb_tok + 2 * nb_n, val2, nb_n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out_tok, pin, nb_tok);
    memcpy(out_len, pin + nb_tok, nb_n);
    if (out_val) memcpy(out_val, pin + nb_tok + nb_n, nb_n);
    if (val2 && out_val2) memcpy(out_val2, pin + nb_tok + 2 * nb_n, nb_n);
    return LRCN_OK;
}

// the n-best beam's device state (lrcn_beam_nbest_batch), allocated on its first call
int nbest_alloc(lrcn_ctx *c) {
    const size_t B = (size_t)c->maxB;
    if (c->nb_store) return LRCN_OK;
    DALLOC(c, c->nb_store, sizeof(int32_t) * B * 2 * LRCN_BEAM_MAXLEN);
    DALLOC(c, c->nb_pool, sizeof(int4) * B);      DALLOC(c, c->nb_img, sizeof(int4) * B);
    DALLOC(c, c->nb_cum, sizeof(float) * B);      DALLOC(c, c->nb_res_score, sizeof(float) * B);
    return LRCN_OK;
}

// ------------------------------------------------------------------------------------------- caption scoring (include/lrcn_score.h)
// LRCN_SCORE_FUSED=0: the logits GEMM writes f32 logits and k_softmax_xent reduces them, at every row count
bool score_fused_on(const lrcn_ctx *c, int R) {
    return !knob_off("LRCN_SCORE_FUSED") && smax_records_on(c, R);
}

// pair_img == NULL: the N x M matrix; else the P pairs.  See lrcn_score.h for the plan; the routes below are chosen once per piece.
int score_impl(lrcn_ctx *c, const float *const p[9], const float *feats, int N, const int32_t *tokens, const int *lens, int M, int Tmax,
               const int32_t *pair_img, const int32_t *pair_cap, int P, float *scores) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    const bool pairs = pair_cap != nullptr || pair_img != nullptr;
    if (!p || !feats || !tokens || !lens || !scores || (pairs && (!pair_img || !pair_cap))) FAIL(c, LRCN_EINVAL, "null argument");
    if (c->nl != 2) FAIL(c, LRCN_EINVAL, "caption scoring needs the two-layer model (LRCN-2f)");
    if (N < 1 || M < 1 || (pairs && P < 1)) FAIL(c, LRCN_EINVAL, "N=%d, M=%d%s must be >= 1", N, M, pairs ? ", P" : "");
    if (!pairs && (int64_t)N * M > INT32_MAX) FAIL(c, LRCN_EINVAL, "N*M = %lld pairs: at most 2^31 - 1", (long long)N * M);
    if (Tmax < 1) FAIL(c, LRCN_EINVAL, "Tmax=%d must be >= 1", Tmax);
    const int V = c->V;
    for (int m = 0; m < M; ++m) {
        if (lens[m] < 1 || lens[m] > LRCN_MAX_T || lens[m] > Tmax) FAIL(c, LRCN_EINVAL, "lens[%d]=%d outside [1, min(Tmax=%d, %d)]", m, lens[m], Tmax, LRCN_MAX_T);
        for (int t = 0; t < lens[m]; ++t)
            if ((unsigned)tokens[(int64_t)t * M + m] >= (unsigned)V) FAIL(c, LRCN_EINVAL, "token (t=%d, m=%d) = %d outside [0, V=%d)", t, m, tokens[(int64_t)t * M + m], V);
    }
    if (pairs)
        for (int q = 0; q < P; ++q)
            if ((unsigned)pair_img[q] >= (unsigned)N || (unsigned)pair_cap[q] >= (unsigned)M)
                FAIL(c, LRCN_EINVAL, "pair %d = (%d, %d) outside N=%d x M=%d", q, pair_img[q], pair_cap[q], N, M);
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, maxB = c->maxB;
    const size_t es = c->esz;
    hipStream_t st = c->stream;
    struct DetScope {   // every GEMM of the call in its ordered form (no float-atomic split-K): a call's scores repeat bit for bit
        lrcn_ctx *c;
        bool prev;
        ~DetScope() { c->opt_det = prev; }
    } det{c, c->opt_det};
    c->opt_det = true;

    // ---- host plan: captions sorted by length (descending, stable); caption step t holds the Ma(t) longest, at rows off[t] .. off[t] + Ma(t)
    std::vector<int> ord(M), rank(M);
    for (int m = 0; m < M; ++m) ord[m] = m;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return lens[a] > lens[b]; });
    for (int j = 0; j < M; ++j) rank[ord[j]] = j;
    const int Smax = lens[ord[0]] + 1;
    std::vector<int64_t> off(Smax + 1, 0);
    std::vector<int> Ma(Smax);
    for (int t = 0, j = M; t < Smax; ++t) {
        while (j > 0 && lens[ord[j - 1]] + 1 <= t) --j;
        Ma[t] = j;
        off[t + 1] = off[t] + j;
    }
    const int64_t Ptot = off[Smax];
    const int64_t Rtot = pairs ? P : (int64_t)N * M;
    // ints: caption-step inputs and targets (each padded by max_B entries: the cell epilogue's GEMM reads up to 256 rows of indices), the
    // sorted order, and for pairs their rows' image, sorted caption and output slot.  A matrix row r is image r % N of sorted caption r / N:
    // its maps are made per piece on the device (k_score_matrix_rows)
    const int64_t n_in = Ptot + maxB, n_int = 2 * n_in + M + (pairs ? 3 * (int64_t)P : 0);
    std::vector<int32_t> hi((size_t)n_int, 0);
    int32_t *h_in = hi.data(), *h_tg = h_in + n_in, *h_ord = h_tg + n_in, *h_img = h_ord + M, *h_cap = h_img + (pairs ? P : 0),
            *h_out = h_cap + (pairs ? P : 0);
    for (int t = 0; t < Smax; ++t)
        for (int j = 0; j < Ma[t]; ++j) {
            const int m = ord[j];
            h_in[off[t] + j] = t == 0 ? LRCN_BOS : tokens[(int64_t)(t - 1) * M + m];
            h_tg[off[t] + j] = t < lens[m] ? tokens[(int64_t)t * M + m] : LRCN_EOS;
        }
    for (int j = 0; j < M; ++j) h_ord[j] = ord[j];
    if (pairs) {
        std::vector<int> q(P);
        for (int i = 0; i < P; ++i) q[i] = i;
        std::stable_sort(q.begin(), q.end(), [&](int a, int b) { return rank[pair_cap[a]] < rank[pair_cap[b]]; });
        for (int i = 0; i < P; ++i) {
            h_img[i] = pair_img[q[i]];
            h_cap[i] = rank[pair_cap[q[i]]];
            h_out[i] = q[i];
        }
    }
    auto steps_of = [&](int64_t row) { return lens[ord[pairs ? h_cap[row] : (int)(row / N)]] + 1; };
    // ---- device arena: the regions of fixed size first, at fixed offsets (A2's K padding must hold zeros; the ride-along rows of the
    // epilogue routes read stale target ids, which must be valid), then the regions whose size depends on the call
    const int64_t ldA2 = c->ldh + c->ldH2;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_A2 = al(es * (size_t)maxB * ldA2), b_i32 = al(sizeof(int32_t) * maxB), b_acc = al(sizeof(double) * maxB),
                 b_terms = al(sizeof(double) * (maxB + 1)), b_int = al(sizeof(int32_t) * n_int), b_P = al(es * Ptot * c->ldh),
                 b_U2 = al(sizeof(float) * (size_t)N * 4 * H2);
    const size_t fixed = 2 * b_A2 + 4 * b_i32 + b_acc + b_terms, need = fixed + b_int + b_P + b_U2;
    HIPCHK(c, hipStreamSynchronize(st));   // a previous score call may still read the arena
    if (need > c->sc_bytes) {
        if (c->sc_arena) (void)hipFree(c->sc_arena);
        c->sc_arena = nullptr;
        c->sc_bytes = 0;
        if (hipMalloc(&c->sc_arena, need) != hipSuccess) FAIL(c, LRCN_ENOMEM, "hipMalloc(%zu) for caption scoring failed", need);
        c->sc_bytes = need;
    }
    char *ap = reinterpret_cast<char *>(c->sc_arena);
    void *A2buf[2] = {ap, ap + b_A2}; ap += 2 * b_A2;
    int32_t *tgt_row = reinterpret_cast<int32_t *>(ap); ap += b_i32;
    int32_t *m_img = reinterpret_cast<int32_t *>(ap), *m_cap = m_img + b_i32 / 4, *m_out = m_cap + b_i32 / 4; ap += 3 * b_i32;
    double *acc = reinterpret_cast<double *>(ap); ap += b_acc;
    double *terms = reinterpret_cast<double *>(ap); ap += b_terms;
    int32_t *d_in = reinterpret_cast<int32_t *>(ap), *d_tg = d_in + n_in, *d_ord = d_tg + n_in, *d_img = d_ord + M,
            *d_cap = d_img + (pairs ? P : 0), *d_out = d_cap + (pairs ? P : 0);
    ap += b_int;
    void *Pst = ap; ap += b_P;
    float *U2 = reinterpret_cast<float *>(ap);
    // every call: zero operands (K padding, first-step h2) and target ids
    HIPCHK(c, hipMemsetAsync(c->sc_arena, 0, 2 * b_A2 + b_i32, st));
    HIPCHK(c, hipMemcpyAsync(d_in, hi.data(), sizeof(int32_t) * n_int, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the host arrays are read before they go out of scope

    int r = decode_tables_alloc(c);
    if (r) return r;
    ShadowNeed sh{};
    sh.dec_tables = true;   // + the interleaved recurrent copies and dec_W2c
    if ((r = prepare_weights(c, p, sh))) return r;
    // ---- caption side: T1, then LSTM-1 and P_t = h1_t Wproj over blocks of max_B sorted captions
    GEMM(c, dt, c->WeT, c->ldE, c->W1x, c->ldX1, c->dec_T1, 4 * H1, V, 4 * H1, E, p[1], true);
    for (int j0 = 0; j0 < M; j0 += maxB) {
        const int Bc = std::min(maxB, M - j0);
        const bool epi = decode_tables_on(c, Bc);
        void *h1c = c->st_h1, *h1n = c->dec_A1;
        float *c1c = c->st_f32[1], *c1n = c->st2_f32[1];
        HIPCHK(c, hipMemsetAsync(h1c, 0, es * (size_t)Bc * c->ldH1, st));
        for (int t = 0; t < Smax && Ma[t] > j0; ++t) {
            const int Ba = std::min(Bc, Ma[t] - j0);
            const int32_t *tok = d_in + off[t] + j0;
            if (epi) {
                if ((r = decode_gates_epi(c, h1c, c->ldH1, c->W1h_gi, H1, c->dec_T1, std::max(Ba, 256), H1, t ? c1c : nullptr, nullptr, c1n, h1n,
                                          c->ldH1, tok)))
                    return r;
            } else {
                k_score_gather_rows(st, c->dec_T1, 4 * H1, tok, Ba, c->st_g);
                if (t) GEMM(c, dt, h1c, c->ldH1, c->W1h, c->ldH1, c->st_g, 4 * H1, Ba, 4 * H1, H1, nullptr, true, true);
                k_lstm_fwd(st, dt, c->st_g, 4 * H1, t ? c1c : nullptr, Ba, H1, c->st_a, c->ld4H1, c1n, h1n, c->ldH1, nullptr);
            }
            GEMM(c, dt, h1n, c->ldH1, c->Wpd, c->ldH1, boff(Pst, (off[t] + j0) * c->ldh, es), c->ldh, Ba, h, H1, nullptr, false);   // lrcn.jl:544
            std::swap(h1c, h1n);
            std::swap(c1c, c1n);
        }
    }
    // ---- image side: U2 = [0 | x_cnn] W2x + b2 per image (x_cnn = feats Wcnn, lrcn.jl:558), in blocks of max_B images
    for (int n0 = 0; n0 < N; n0 += maxB) {
        const int nc = std::min(maxB, N - n0);
        k_transpose(st, dt, 1, feats + n0, N, LRCN_CNNOUT, nc, c->F, LRCN_CNNOUT, 0);
        GEMM(c, dt, c->F, LRCN_CNNOUT, c->Wcd, LRCN_CNNOUT, c->dxcnn, c->ldh, nc, h, LRCN_CNNOUT, nullptr, true);
        HIPCHK(c, hipMemsetAsync(c->dec_Aimg, 0, es * (size_t)nc * c->ldH2, st));
        DropSpec none{};
        k_concat_x2(st, dt, c->dec_Aimg, c->ldH2, c->dxcnn, c->ldh, 1, nc, h, h, none);
        GEMM(c, dt, c->dec_Aimg, c->ldH2, c->W2x, c->ldH2, U2 + (int64_t)n0 * 4 * H2, 4 * H2, nc, 4 * H2, H2, p[3], true);
    }
    // ---- pair side: pieces of at most max_B caption-major rows
    for (int64_t r0 = 0; r0 < Rtot; r0 += maxB) {
        const int R = (int)std::min<int64_t>(maxB, Rtot - r0);
        const bool epi = decode_tables_on(c, R), fused = score_fused_on(c, R);
        const int Sp = steps_of(r0);
        void *A2c = A2buf[0], *A2n = A2buf[1];
        float *c2c = c->st_f32[3], *c2n = c->st2_f32[3];
        const int32_t *img = d_img + r0, *cap = d_cap + r0, *outi = d_out + r0;
        if (!pairs) {
            k_score_matrix_rows(st, r0, R, N, d_ord, m_img, m_cap, m_out);
            img = m_img; cap = m_cap; outi = m_out;
        }
        HIPCHK(c, hipMemsetAsync(acc, 0, sizeof(double) * R, st));
        int Rt = R;
        for (int t = 0; t < Sp; ++t) {
            while (Rt > 0 && steps_of(r0 + Rt - 1) <= t) --Rt;
            // rows past Rt (inactive for good) ride along up to 256 in the epilogue routes: their operands are finite, their results unread
            const int Mg = epi ? std::max(Rt, 256) : Rt, Ml = fused ? std::max(Rt, 256) : Rt;
            k_score_prep(st, dt, A2c, ldA2, boff(Pst, off[t] * c->ldh, es), c->ldh, cap, Rt, h, t == 0 ? H2 : 0, c->ldh, d_tg + off[t], tgt_row);
            void *h2n = boff(A2n, c->ldh, es);
            if (epi) {
                if ((r = decode_gates_epi(c, A2c, ldA2, c->dec_W2c, (int)ldA2, U2, Mg, H2, t ? c2c : nullptr, nullptr, c2n, h2n, ldA2, img))) return r;
            } else {
                k_score_gather_rows(st, U2, 4 * H2, img, Rt, c->st_g);
                GEMM(c, dt, A2c, ldA2, c->W2x, c->ldH2, c->st_g, 4 * H2, Rt, 4 * H2, h, nullptr, true, true);   // P_t: the left h columns of W2x
                if (t) GEMM(c, dt, boff(A2c, c->ldh, es), ldA2, c->W2h, c->ldH2, c->st_g, 4 * H2, Rt, 4 * H2, H2, nullptr, true, true);
                k_lstm_fwd(st, dt, c->st_g, 4 * H2, t ? c2c : nullptr, Rt, H2, c->st_a, c->ld4H2, c2n, h2n, ldA2, nullptr);
            }
            if (fused) {
                SmaxEpi pick{};
                pick.tgt = tgt_row;
                if ((r = logits_records(c, h2n, ldA2, p[8], Ml, GEMM_OUT_SMAX_PICK, pick))) return r;   // lrcn.jl:550, log-softmax pick epilogue
                if (!k_score_pick_merge(st, c->smax_part, smax_nrec(c), Rt, acc)) FAIL(c, LRCN_EINVAL, "score merge: %d records per row", smax_nrec(c));
            } else {
                GEMM(c, dt, h2n, ldA2, c->Wod, c->ldH2, c->st_logits, c->ldV, Rt, V, H2, p[8], true);   // lrcn.jl:550
                XentCall x{};  // PLAIN: the rows' terms, then their sum behind them
                x.logits = c->st_logits; x.ld_l = c->ldV; x.tgt = tgt_row; x.M = Rt; x.V = V; x.scale = 1.0f;
                x.sum = terms + maxB; x.rows = terms;
                k_softmax_xent(st, dt, x);
                k_score_acc(st, terms, Rt, acc);
            }
            std::swap(A2c, A2n);
            std::swap(c2c, c2n);
        }
        k_score_scatter(st, acc, outi, R, scores);
    }
    KCHK(c, "score");
    return LRCN_OK;
}

}  // namespace

extern "C" {

int lrcn_beam_search(lrcn_ctx *c, const float *const p[9], const float *feat, int K, int nword, int32_t *out_tokens, int *out_len,
                     float *out_prob) {
    DeviceGuard dg(c);
    if (!c || !p || !feat || !out_tokens || !out_len) return LRCN_EINVAL;
    if (K < 1 || K > 32 || K > c->maxB || K > c->V) FAIL(c, LRCN_EINVAL, "beam width K=%d must be in [1, min(32, max_B=%d, V=%d)]", K, c->maxB, c->V);
    if (nword < 1 || nword > 256) FAIL(c, LRCN_EINVAL, "nword=%d outside [1,256]", nword);
    const int dt = c->dt, E = c->E, H1 = c->H1, H2 = c->H2, h = c->h;
    hipStream_t st = c->stream;
    int r = prepare_weights(c, p);   // the forward shadows alone
    if (r) return r;
    // input = input * param[end-3]  (lrcn.jl:611), replicated to K rows
    k_cast_rows(st, dt, feat, LRCN_CNNOUT, 1, LRCN_CNNOUT, c->F, LRCN_CNNOUT);
    for (int i = 1; i < K; ++i)
        HIPCHK(c, hipMemcpyAsync(boff(c->F, (int64_t)i * LRCN_CNNOUT, c->esz), c->F, c->esz * LRCN_CNNOUT, hipMemcpyDeviceToDevice, st));
    GEMM(c, dt, c->F, LRCN_CNNOUT, c->Wcd, LRCN_CNNOUT, c->xcnn, c->ldh, K, h, LRCN_CNNOUT, nullptr, true);
    const int Hs[4] = {H1, H1, H2, H2};
    for (int i = 0; i < 4; ++i) HIPCHK(c, hipMemsetAsync(c->st_f32[i], 0, sizeof(float) * (size_t)K * Hs[i], st));
    struct Hyp {
        std::vector<int32_t> seq;
        float p;
    };
    std::vector<Hyp> x(K);
    for (auto &hy : x) {
        hy.seq = {LRCN_BOS};
        hy.p = 1.0f;
    }
    std::vector<int32_t> last(K), topi((size_t)K * K), parent(K);
    std::vector<float> topv((size_t)K * K);
    DropSpec none{};
    for (int current = 1;; ++current) {
        for (int i = 0; i < K; ++i) last[i] = x[i].seq.back();
        HIPCHK(c, hipMemcpyAsync(c->st_parent, last.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, st));
        k_embed_gather(st, dt, c->WeT, c->ldE, c->st_parent, 1, K, E, none, c->st_x, c->ldX1);  // lrcn.jl:650
        r = step_internal(c, p, K, none);                                                    // lrcn.jl:651 (K hypotheses batched)
        if (r) return r;
        topk_rows(c, K, K, false);                                                           // :652, :655-656 on device
        HIPCHK(c, hipMemcpyAsync(topi.data(), c->st_topi, sizeof(int32_t) * K * K, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(topv.data(), c->st_topv, sizeof(float) * K * K, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        // candidates (lrcn.jl:657-664): step 1 expands hypothesis 1 only
        const int nexp = current == 1 ? 1 : K;
        std::vector<Hyp> cand;
        std::vector<int> cparent;
        for (int i = 0; i < nexp; ++i)
            for (int j = 0; j < K; ++j) {
                Hyp hy;
                hy.seq = x[i].seq;
                hy.seq.push_back(topi[(size_t)i * K + j]);
                hy.p = topv[(size_t)i * K + j] * x[i].p;
                cand.push_back(std::move(hy));
                cparent.push_back(i);
            }
        // stable descending sort by probability (lrcn.jl:667)
        std::vector<int> order(cand.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cand[a].p > cand[b].p; });
        std::vector<Hyp> xs(K);
        for (int i = 0; i < K; ++i) xs[i] = cand[order[i]];
        const bool done = xs[0].seq.back() == LRCN_EOS || current > nword;  // :670
        if (done) {
            x.swap(xs);
            break;
        }
        for (int i = 0; i < K; ++i) parent[i] = cparent[order[i]];  // :673-676
        HIPCHK(c, hipMemcpyAsync(c->st_parent, parent.data(), sizeof(int32_t) * K, hipMemcpyHostToDevice, st));
        for (int i = 0; i < 4; ++i) {
            k_gather_rows_f32(st, c->st_f32[i], Hs[i], c->st_parent, K, Hs[i], c->st2_f32[i]);
            std::swap(c->st_f32[i], c->st2_f32[i]);
        }
        HIPCHK(c, hipStreamSynchronize(st));  // parent/last host vectors are reused next iteration
        x.swap(xs);
    }
    const int n = (int)x[0].seq.size();
    memcpy(out_tokens, x[0].seq.data(), sizeof(int32_t) * n);
    *out_len = n;
    if (out_prob) *out_prob = x[0].p;
    return LRCN_OK;
}

// generate/beam_search for N images at once (lrcn.jl:585-678 per image; the reference decodes one image at a time with K
// sequential batch-1 lrcn() calls and a device->host copy of V floats per hypothesis per step).  Here the N*K hypotheses of all
// images are the rows of ONE batched lrcn() step (decode_begin / decode_step, shared with lrcn_sample_batch); softmax, top-K,
// candidate ordering, history update and the stop test run on the device (beam_update_kernel); the host only polls a done-counter
// every few steps.  Per image the result is what lrcn_beam_search returns (tests/test_gpu_lstm_parity.py).  feats: N x 4096
// column-major; out_tokens: [N][nword + 2] (bos first), out_len[N], out_prob[N] (may be NULL) on the HOST.
int lrcn_beam_search_batch(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int K, int nword, int32_t *out_tokens,
                           int *out_len, float *out_prob) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || !out_tokens || !out_len) return LRCN_EINVAL;
    if (K < 1 || K > 32 || K > c->V) FAIL(c, LRCN_EINVAL, "beam width K=%d must be in [1, min(32, V=%d)]", K, c->V);
    if (N < 1 || (int64_t)N * K > c->maxB) FAIL(c, LRCN_EINVAL, "N*K = %d*%d exceeds max_B = %d", N, K, c->maxB);
    if (nword < 1 || nword + 2 > LRCN_BEAM_MAXLEN) FAIL(c, LRCN_EINVAL, "nword=%d outside [1,%d]", nword, LRCN_BEAM_MAXLEN - 2);
    const int R = N * K, Lh = nword + 2;
    hipStream_t st = c->stream;
    const DecodeRoute rt = decode_route(c, R, K);
    int r = decode_begin(c, p, feats, N, K, rt);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->bs_done, 0, sizeof(int32_t) * N, st));
    HIPCHK(c, hipMemsetAsync(c->bs_ndone, 0, sizeof(int32_t), st));
    k_beam_init(st, c->bs_seq[0], c->bs_last, c->bs_p, R, Lh, LRCN_BOS);  // histories = [bos], probabilities 1, next input = bos
    DecodeTail tail{};   // :652, :655-656 (in the logits GEMM's epilogue + merge on the record route)
    tail.kind = DecodeTail::TOPK;
    tail.K = K;
    tail.records = rt.smax;
    int cur = 0;
    for (int current = 1; current <= nword + 1; ++current) {
        if ((r = decode_step(c, p, R, rt, current, tail))) return r;   // :650-651, all N*K hypotheses batched
        k_beam_update(st, c->st_topi, c->st_topv, c->bs_seq[cur], c->bs_seq[cur ^ 1], c->bs_p, c->st_parent, c->bs_last, c->bs_done,
                      c->bs_ndone, c->bs_res_tok, c->bs_res_len, c->bs_res_p, N, K, Lh, current, nword, LRCN_EOS);
        cur ^= 1;
        if (!rt.epi) follow_parents(c, R);   // :673-676
        bool done = false;   // every image finished early?
        if ((current & 3) == 0 && current <= nword && (r = decode_poll_done(c, N, done))) return r;
        if (done) break;
    }
    KCHK(c, "beam_search_batch");
    return decode_results_to_host(c, c->bs_res_tok, c->bs_res_len, c->bs_res_p, N, Lh, out_tokens, out_len, out_prob);
}

// Test entry (include/lrcn_decode_debug.h): the batched decode's own begin and step on the route decode_route picks, fed the caller's
// tokens and parents instead of a beam's or a sampler's, the states and f32 logits copied out after every step.  The plain step reads no
// parent, so its states are gathered in front of the step -- what lrcn_beam_search_batch does behind the step before.
int lrcn_debug_decode_steps(lrcn_ctx *c, lrcn_decode_debug *d) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (!d) FAIL(c, LRCN_EINVAL, "null argument");
    const bool two = c->nl == 2;
    if (!d->params || !d->feats || !d->tokens || !d->parents || !d->h1 || !d->c1 || !d->logits || (two && (!d->h2 || !d->c2)))
        FAIL(c, LRCN_EINVAL, "null argument");
    int64_t sz[9];
    ctx_sizes(c, sz);
    for (int i = 0; i < 9; ++i)
        if (sz[i] > 0 && !d->params[i]) FAIL(c, LRCN_EINVAL, "null parameter array %d", i);
    if (d->N < 1 || d->per_image < 1 || d->steps < 1) FAIL(c, LRCN_EINVAL, "N=%d, per_image=%d, steps=%d must be >= 1", d->N, d->per_image, d->steps);
    if ((int64_t)d->N * d->per_image > c->maxB) FAIL(c, LRCN_EINVAL, "N*per_image = %d*%d exceeds max_B = %d", d->N, d->per_image, c->maxB);
    const int N = d->N, R = d->N * d->per_image, S = d->steps, H1 = c->H1, H2 = c->H2, V = c->V;
    for (int s = 0; s < S; ++s)
        for (int r = 0; r < R; ++r) {
            const int32_t tk = d->tokens[(int64_t)s * R + r], pa = d->parents[(int64_t)s * R + r];
            if ((unsigned)tk >= (unsigned)V) FAIL(c, LRCN_EINVAL, "token (step %d, row %d) = %d outside [0, V=%d)", s, r, tk, V);
            if (s > 0 && (unsigned)pa >= (unsigned)R) FAIL(c, LRCN_EINVAL, "parent (step %d, row %d) = %d outside [0, R=%d)", s, r, pa, R);
        }
    const float *const *p = d->params;
    const size_t es = c->esz;
    hipStream_t st = c->stream;
    const DecodeRoute rt = decode_route(c, R, 0);
    int r = decode_begin(c, p, d->feats, N, d->per_image, rt);
    if (r) return r;
    DecodeTail tail{};   // LOGITS: f32 logits in st_logits on every route
    for (int s = 0; s < S; ++s) {
        HIPCHK(c, hipMemcpyAsync(c->bs_last, d->tokens + (int64_t)s * R, sizeof(int32_t) * R, hipMemcpyHostToDevice, st));
        if (s > 0) {
            HIPCHK(c, hipMemcpyAsync(c->st_parent, d->parents + (int64_t)s * R, sizeof(int32_t) * R, hipMemcpyHostToDevice, st));
            if (!rt.epi) follow_parents(c, R);   // :673-676
        }
        if ((r = decode_step(c, p, R, rt, s + 1, tail))) return r;
        // this step's h: the epilogues' own buffers, or the h blocks of the plain step's [x | h] operands
        const void *h1 = rt.epi ? c->st_h1 : boff(c->st_xh1, c->ldX1, es), *h2 = rt.epi ? c->st_h2 : boff(c->st_xh2, c->ldH2, es);
        const int64_t ld1 = rt.epi ? c->ldH1 : c->ldXH1, ld2 = rt.epi ? c->ldH2 : c->ldXH2;
        HIPCHK(c, hipMemcpyAsync(d->c1 + (int64_t)s * R * H1, c->st_f32[1], sizeof(float) * (size_t)R * H1, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpy2DAsync(boff(d->h1, (int64_t)s * R * H1, es), es * H1, h1, es * ld1, es * H1, R, hipMemcpyDeviceToDevice, st));
        if (two) {
            HIPCHK(c, hipMemcpyAsync(d->c2 + (int64_t)s * R * H2, c->st_f32[3], sizeof(float) * (size_t)R * H2, hipMemcpyDeviceToDevice, st));
            HIPCHK(c, hipMemcpy2DAsync(boff(d->h2, (int64_t)s * R * H2, es), es * H2, h2, es * ld2, es * H2, R, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(c, hipMemcpy2DAsync(d->logits + (int64_t)s * R * V, sizeof(float) * V, c->st_logits, sizeof(float) * c->ldV, sizeof(float) * V, R,
                                   hipMemcpyDeviceToDevice, st));
    }
    KCHK(c, "debug_decode_steps");
    HIPCHK(c, hipStreamSynchronize(st));
    d->route = rt.tables ? 2 : rt.epi ? 1 : 0;
    return LRCN_OK;
}

}  // extern "C"
namespace {

// Sampled generation (include/lrcn_sample.h; the sample() path of lrcn.jl:613-621, 680-687): the batched decode of lrcn_beam_search_batch
// (decode_begin / decode_step on the route decode_route picks) with R = N*S independent rows instead of N*K beams: the parent index is the
// identity, and the per-step choice is a Gumbel-max draw per row (sample.hip) instead of top-K and a beam reorder.  Where the beam's logits
// GEMM reduces to top-K records (decode_smax_on), top_k = 0 reduces to Gumbel records instead (GEMM_OUT_SMAX_GUMBEL) and 1 <= top_k < SMAX_KC
// draws among the top-K records' best columns; otherwise the logits reach st_logits and one workgroup per row draws (LRCN_DECODE_SMAX=0
// forces that form).
// nucleus (include/lrcn_nucleus.h; top_p < 1 or top_k > 32): the selection needs the whole row -- a record keeps SMAX_KC columns of its 128,
// the Gumbel record one -- so the records tail is off whatever the router says (the cell epilogue and the tables stay as it picks them), the
// logits reach st_logits and sample_nucleus_kernel selects and draws; d_count [R][nword + 1] (may be NULL) takes its admitted-set sizes.
int sample_impl(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int S, int nword, float temperature, int top_k, float top_p,
                bool nucleus, uint64_t seed, int32_t *out_tokens, int *out_len, float *out_logp, int32_t *d_count) {
    const int R = N * S, Lh = nword + 2, nrec = smax_nrec(c);
    hipStream_t st = c->stream;
    DecodeRoute rt = decode_route(c, R, nucleus ? 0 : top_k);   // smax: top_k < SMAX_KC
    if (nucleus) rt.smax = false;
    int r = decode_begin(c, p, feats, N, S, rt);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->bs_ndone, 0, sizeof(int32_t), st));
    if (nucleus && d_count) HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(int32_t) * (size_t)R * (nword + 1), st));
    SampleState ss{c->bs_seq[0], c->bs_last, c->bs_done, c->bs_res_len, c->bs_ndone, c->bs_p, Lh, 0, nword, LRCN_EOS};
    k_sample_init(st, ss, R, LRCN_BOS);   // histories = [bos], log-likelihoods 0, next input = bos
    k_row_div(st, c->st_parent, R, 1);    // every row continues its own state: the plain step's in-place update needs no gather
    DecodeTail tail{};
    if (rt.smax && top_k == 0) {
        tail.kind = DecodeTail::GUMBEL;
        tail.draw.temp = temperature;
        tail.draw.key0 = (uint32_t)seed;
        tail.draw.key1 = (uint32_t)(seed >> 32);
        tail.draw.S = S;
    } else if (rt.smax) {
        tail.kind = DecodeTail::RECORDS;
    }
    for (int current = 1; current <= nword + 1; ++current) {
        ss.current = current;
        tail.draw.current = current;
        if ((r = decode_step(c, p, R, rt, current, tail))) return r;
        if (tail.kind == DecodeTail::GUMBEL) {
            if (!k_sample_gumbel_merge(st, c->smax_part, nrec, R, ss)) FAIL(c, LRCN_EINVAL, "sample merge: %d records per row", nrec);
        } else if (tail.kind == DecodeTail::RECORDS) {
            if (!k_sample_topk_merge(st, c->smax_part, nrec, R, top_k, temperature, seed, S, ss)) FAIL(c, LRCN_EINVAL, "sample top-k merge: top_k = %d, %d records", top_k, nrec);
        } else if (nucleus) {
            k_sample_nucleus(st, c->st_logits, c->ldV, R, c->V, S, current, temperature, top_k, top_p, seed, &ss,
                             d_count ? d_count + (current - 1) : nullptr, nword + 1, nullptr, nullptr);
        } else {
            k_sample_rows(st, c->st_logits, c->ldV, R, c->V, top_k, temperature, seed, S, ss);
        }
        bool done = false;   // every row finished early?
        if ((current & 3) == 0 && current <= nword && (r = decode_poll_done(c, R, done))) return r;
        if (done) break;
    }
    KCHK(c, "sample_batch");
    return decode_results_to_host(c, c->bs_seq[0], c->bs_res_len, c->bs_p, R, Lh, out_tokens, out_len, out_logp);
}
}  // namespace
extern "C" {

int lrcn_sample_batch(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int S, int nword, float temperature, int top_k,
                      uint64_t seed, int32_t *out_tokens, int *out_len, float *out_logp) {
    DeviceGuard dg(c);
    if (!c || !p || !feats || !out_tokens || !out_len) return LRCN_EINVAL;
    if (N < 1 || S < 1 || (int64_t)N * S > c->maxB) FAIL(c, LRCN_EINVAL, "N*S = %d*%d must be in [1, max_B = %d]", N, S, c->maxB);
    if (!std::isfinite(temperature) || temperature < 0.0f) FAIL(c, LRCN_EINVAL, "temperature=%g must be finite and >= 0", (double)temperature);
    if (top_k < 0 || top_k > 32 || top_k > c->V) FAIL(c, LRCN_EINVAL, "top_k=%d must be in [0, min(32, V=%d)]", top_k, c->V);
    if (nword < 1 || nword + 2 > LRCN_BEAM_MAXLEN) FAIL(c, LRCN_EINVAL, "nword=%d outside [1,%d]", nword, LRCN_BEAM_MAXLEN - 2);
    return sample_impl(c, p, feats, N, S, nword, temperature, top_k, 1.0f, false, seed, out_tokens, out_len, out_logp, nullptr);
}

// include/lrcn_nucleus.h.  top_p == 1 with top_k <= 32, and every greedy call (T = 0: neither cut has an effect), are lrcn_sample_batch's
// own path; their admitted-set sizes (|A_k| at every live step) are filled in on the host from the lengths.
int lrcn_sample_batch_p(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int S, int nword, float temperature, int top_k,
                        float top_p, uint64_t seed, int32_t *out_tokens, int *out_len, float *out_logp, int32_t *out_count) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (!p || !feats || !out_tokens || !out_len) FAIL(c, LRCN_EINVAL, "null argument");
    if (N < 1 || S < 1 || (int64_t)N * S > c->maxB) FAIL(c, LRCN_EINVAL, "N*S = %d*%d must be in [1, max_B = %d]", N, S, c->maxB);
    if (!std::isfinite(temperature) || temperature < 0.0f) FAIL(c, LRCN_EINVAL, "temperature=%g must be finite and >= 0", (double)temperature);
    if (top_k < 0 || top_k > c->V) FAIL(c, LRCN_EINVAL, "top_k=%d must be in [0, V=%d]", top_k, c->V);
    if (!(top_p > 0.0f && top_p <= 1.0f)) FAIL(c, LRCN_EINVAL, "top_p=%g must be in (0, 1]", (double)top_p);
    if (nword < 1 || nword + 2 > LRCN_BEAM_MAXLEN) FAIL(c, LRCN_EINVAL, "nword=%d outside [1,%d]", nword, LRCN_BEAM_MAXLEN - 2);
    const int R = N * S, nstep = nword + 1;
    const bool greedy = temperature == 0.0f, nucleus = !greedy && (top_p < 1.0f || top_k > 32);
    if (nucleus && out_count && !c->smp_count) DALLOC(c, c->smp_count, sizeof(int32_t) * (size_t)c->maxB * (LRCN_BEAM_MAXLEN - 1));
    int r = sample_impl(c, p, feats, N, S, nword, temperature, greedy ? 0 : top_k, top_p, nucleus, seed, out_tokens, out_len, out_logp,
                    nucleus && out_count ? c->smp_count : nullptr);
    if (r || !out_count) return r;
    if (!nucleus) {
        const int nk = greedy || top_k == 0 ? c->V : top_k;
        for (int row = 0; row < R; ++row)
            for (int t = 0; t < nstep; ++t) out_count[(size_t)row * nstep + t] = t < out_len[row] - 1 ? nk : 0;
        return LRCN_OK;
    }
    const size_t nb = sizeof(int32_t) * (size_t)R * nstep;
    if ((r = pin_reserve(c, nb))) return r;
    HIPCHK(c, hipMemcpyAsync(c->pin, c->smp_count, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out_count, c->pin, nb);
    return LRCN_OK;
}

int lrcn_sample_logits(lrcn_ctx *c, const float *logits, int64_t ld, int R, int V, int S, int current, float temperature, int top_k, float top_p,
                       uint64_t seed, int32_t *out_tok, float *out_logp, int32_t *out_count) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (!logits || !out_tok) FAIL(c, LRCN_EINVAL, "null argument");
    if (R < 1 || V < 1 || S < 1 || ld < V) FAIL(c, LRCN_EINVAL, "R=%d, V=%d, S=%d must be >= 1 and ld=%lld >= V", R, V, S, (long long)ld);
    if (current < 0) FAIL(c, LRCN_EINVAL, "current=%d must be >= 0", current);
    if (!std::isfinite(temperature) || temperature < 0.0f) FAIL(c, LRCN_EINVAL, "temperature=%g must be finite and >= 0", (double)temperature);
    if (top_k < 0 || top_k > V) FAIL(c, LRCN_EINVAL, "top_k=%d must be in [0, V=%d]", top_k, V);
    if (!(top_p > 0.0f && top_p <= 1.0f)) FAIL(c, LRCN_EINVAL, "top_p=%g must be in (0, 1]", (double)top_p);
    k_sample_nucleus(c->stream, logits, ld, R, V, S, current, temperature, top_k, top_p, seed, nullptr, out_count, 1, out_tok, out_logp);
    KCHK(c, "sample_logits");
    return LRCN_OK;
}

// ---------------------------------------------------------------------------- constrained top-K (include/lrcn_constrain.h, constrain.hip)
// The checks of a constraint set for a vocabulary of V, a width K and histories of at most `words` words (the feasibility bound
// V - nbanned - 1 - words >= K; K = 0: not asked); max_min_len < 0: min_len is not bounded.  bits: the list as a bitmap of (V + 31) / 32 words.
static int constraints_check(lrcn_ctx *c, const lrcn_constraints *cons, int V, int K, int words, int max_min_len, std::vector<uint32_t> &bits) {
    if (cons->nbanned < 0 || cons->min_len < 0 || cons->no_repeat_ngram < 0)
        FAIL(c, LRCN_EINVAL, "constraints: nbanned=%d, min_len=%d, no_repeat_ngram=%d must be >= 0", cons->nbanned, cons->min_len, cons->no_repeat_ngram);
    if (cons->nbanned > 0 && !cons->banned) FAIL(c, LRCN_EINVAL, "constraints: nbanned=%d with a NULL list", cons->nbanned);
    if (max_min_len >= 0 && cons->min_len > max_min_len) FAIL(c, LRCN_EINVAL, "constraints: min_len=%d exceeds nword=%d", cons->min_len, max_min_len);
    bits.assign(((size_t)V + 31) / 32, 0u);
    for (int q = 0; q < cons->nbanned; ++q) {
        const int32_t v = cons->banned[q];
        if (v < 1 || v >= V) FAIL(c, LRCN_EINVAL, "constraints: banned[%d]=%d outside [1, V=%d) (eos: use min_len)", q, v, V);
        if ((bits[v >> 5] >> (v & 31)) & 1u) FAIL(c, LRCN_EINVAL, "constraints: banned[%d]=%d is a duplicate", q, v);
        bits[v >> 5] |= 1u << (v & 31);
    }
    if (K > 0 && (int64_t)V - cons->nbanned - 1 - words < K)
        FAIL(c, LRCN_EINVAL, "constraints: V - nbanned - 1 - %d = %lld leaves fewer than K=%d allowed words", words,
             (long long)V - cons->nbanned - 1 - words, K);
    return LRCN_OK;
}
// the bitmap into the context's buffer, with `scratch` bytes behind it (*scratch_out); the call's only wait besides its results
static int constraints_upload(lrcn_ctx *c, const std::vector<uint32_t> &bits, size_t scratch, float **scratch_out) {
    const size_t b_bits = (sizeof(uint32_t) * bits.size() + 255) & ~(size_t)255, need = b_bits + scratch;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // a previous call may still read the buffer
    if (need > c->cn_bytes) {
        if (c->cn_arena) (void)hipFree(c->cn_arena);
        c->cn_arena = nullptr;
        c->cn_bytes = 0;
        if (hipMalloc(&c->cn_arena, need) != hipSuccess) FAIL(c, LRCN_ENOMEM, "hipMalloc(%zu) for the constraints failed", need);
        c->cn_bytes = need;
    }
    HIPCHK(c, hipMemcpyAsync(c->cn_arena, bits.data(), sizeof(uint32_t) * bits.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vector is read before it goes out of scope
    if (scratch_out) *scratch_out = reinterpret_cast<float *>(reinterpret_cast<char *>(c->cn_arena) + b_bits);
    return LRCN_OK;
}
// topk_rows' LOGP form on the allowed columns: one pass where the rows kernel fits, else log-softmax into `scratch` [R][ld], -inf over the
// banned columns, and the plain top-K
static void constrained_topk_rows(lrcn_ctx *c, const float *logits, int64_t ld, int R, int V, int K, const ConstrainArgs &a, float *scratch,
                                  int32_t *idx, float *val) {
    if (k_constrained_topk_rows(c->stream, logits, ld, R, V, K, a, idx, val)) return;
    k_log_softmax_rows(c->stream, logits, ld, R, V, scratch, ld);
    k_constrain_mask_rows(c->stream, scratch, ld, R, V, a);
    k_topk_rows(c->stream, scratch, ld, R, V, K, idx, val);
}

// -------------------------------------------------------------------------------------------- forced words (include/lrcn_forced.h)
static_assert(kForcedMaxSets == LRCN_FORCED_MAXSETS && kForcedMaxAlt == LRCN_FORCED_MAXALT, "ForcedArgs holds the header's limits");
// The id rules of n_img images' sets words [n_img][C][A] against a vocabulary of V and the ban bitmap `bits`: an id is negative (no word)
// or in [1, V), occurs once within its image and is not banned.  table: the device form, [n_img][C*A] with -1 for no word.
static int forced_check(lrcn_ctx *c, const int32_t *words, int n_img, int C, int A, int V, const std::vector<uint32_t> &bits,
                        std::vector<int32_t> &table) {
    const int CA = C * A;
    table.assign((size_t)n_img * CA, -1);
    for (int n = 0; n < n_img; ++n)
        for (int q = 0; q < CA; ++q) {
            const int32_t v = words[(size_t)n * CA + q];
            if (v < 0) continue;
            if (v < 1 || v >= V) FAIL(c, LRCN_EINVAL, "forced words: image %d, set %d: id %d outside [1, V=%d)", n, q / A, v, V);
            if ((bits[v >> 5] >> (v & 31)) & 1u) FAIL(c, LRCN_EINVAL, "forced words: image %d, set %d: id %d is banned", n, q / A, v);
            for (int o = 0; o < q; ++o)
                if (table[(size_t)n * CA + o] == v) FAIL(c, LRCN_EINVAL, "forced words: image %d: id %d occurs twice", n, v);
            table[(size_t)n * CA + q] = v;
        }
    return LRCN_OK;
}
// the word table behind the bitmap in the constraint arena (constraints_upload has made room at `dst`)
static int forced_upload(lrcn_ctx *c, const std::vector<int32_t> &table, int32_t *dst) {
    if (table.empty()) return LRCN_OK;
    HIPCHK(c, hipMemcpyAsync(dst, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // the host vector is read before it goes out of scope
    return LRCN_OK;
}
// constrained_topk_rows for rows that know their state: the stay proposals, the move values and the states
static void forced_topk_rows(lrcn_ctx *c, const float *logits, int64_t ld, int R, int V, int K, const ConstrainArgs &a, const ForcedArgs &f,
                             float *scratch, int32_t *idx, float *val, float *move, int32_t *state) {
    if (k_forced_topk_rows(c->stream, logits, ld, R, V, K, a, f, idx, val, move, state)) return;
    k_log_softmax_rows(c->stream, logits, ld, R, V, scratch, ld);
    k_forced_mask_rows(c->stream, scratch, ld, R, V, a, f, move, state);
    k_topk_rows(c->stream, scratch, ld, R, V, K, idx, val);
}
// decode_results_to_host for a forced call: the results are in the first K of every image's `per` rows, and the host arrays are [N][K]
static int forced_results_to_host(lrcn_ctx *c, int N, int K, int per, int Lh, int32_t *out_tok, int *out_len, float *out_logp, float *out_score) {
    const size_t w_tok = sizeof(int32_t) * (size_t)K * Lh, w_n = sizeof(int32_t) * (size_t)K, nb_tok = w_tok * N, nb_n = w_n * N;
    int r = pin_reserve(c, nb_tok + 3 * nb_n);
    if (r) return r;
    unsigned char *pin = reinterpret_cast<unsigned char *>(c->pin);
    HIPCHK(c, hipMemcpy2DAsync(pin, w_tok, c->bs_res_tok, sizeof(int32_t) * (size_t)per * Lh, w_tok, N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(pin + nb_tok, w_n, c->bs_res_len, sizeof(int32_t) * (size_t)per, w_n, N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(pin + nb_tok + nb_n, w_n, c->bs_res_p, sizeof(float) * (size_t)per, w_n, N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(pin + nb_tok + 2 * nb_n, w_n, c->nb_res_score, sizeof(float) * (size_t)per, w_n, N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out_tok, pin, nb_tok);
    memcpy(out_len, pin + nb_tok, nb_n);
    if (out_logp) memcpy(out_logp, pin + nb_tok + nb_n, nb_n);
    if (out_score) memcpy(out_score, pin + nb_tok + 2 * nb_n, nb_n);
    return LRCN_OK;
}

// The n-best beam search (include/lrcn_nbest.h): the batched decode of lrcn_beam_search_batch (decode_begin / decode_step on the route
// decode_route picks, N*K rows) with log-probability top-K (the LOGP forms of the records merge and the rows kernel) and its own per-step
// bookkeeping (nbest.hip): live slots in log space, a pool of finished hypotheses with length normalisation, the exact early stop.
// G > 0 (0: the n-best beam): diverse beam search (include/lrcn_diverse.h) -- the same decode and top-K at the full width K, the bookkeeping
// of diverse.hip.
// cons != NULL (include/lrcn_constrain.h; its entry point passes NULL for an empty set): the record epilogue is off, as for a nucleus call
// of sample_impl, the step leaves f32 logits, and constrained_topk_rows on them and the histories in bs_seq takes topk_rows' place.
// ens != NULL (include/lrcn_ensemble.h; its entry point has checked the members): c and p are member 0, the leader.  Every member runs the
// decode -- begin and step, f32 logits -- in its own context on its own route, one launch mixes their st_logits into the leader's ens_mix,
// and from there on the call is the constrained one on the leader (an empty constraint set if cons == NULL) with the mixture for logits.
// The other members get the leader's parents and next tokens by device copies behind the bookkeeping kernel.
// forced != NULL (include/lrcn_forced.h; its entry point has checked C and A and passes NULL for no sets; G = 0, no ensemble): an image owns
// S = 2^C banks of K rows, the decode runs on N*S*K rows on the route of that row count, forced_topk_rows takes constrained_topk_rows'
// place and forced.hip's bookkeeping nbest.hip's; the results are gathered from the first K rows of every image.
static_assert(kEnsembleMax == LRCN_ENSEMBLE_MAX, "EnsembleMixArgs holds LRCN_ENSEMBLE_MAX members");
struct Ensemble {
    int M;
    lrcn_ctx *const *ctx;
    const float *const *const *p;
    float w[LRCN_ENSEMBLE_MAX];   // normalised
    bool log_mean;
};
// a failure inside member m's context, told where the caller looks: the leader's last error
static int member_fail(lrcn_ctx *c, const lrcn_ctx *cm, int m, int r) {
    if (cm != c) c->err = "ensemble member " + std::to_string(m) + ": " + cm->err;
    return r;
}
static int pool_beam_impl(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int K, int G, float lambda, int nword, float alpha,
                          int32_t *out_tokens, int *out_len, float *out_logp, float *out_score, const lrcn_constraints *cons = nullptr,
                          const Ensemble *ens = nullptr, const lrcn_forced *forced = nullptr) {
    if (!p || !feats || !out_tokens || !out_len) FAIL(c, LRCN_EINVAL, "null argument");
    if (K < 1 || K > 32 || K > c->V) FAIL(c, LRCN_EINVAL, "beam width K=%d must be in [1, min(32, V=%d)]", K, c->V);
    if (N < 1 || (int64_t)N * K > c->maxB) FAIL(c, LRCN_EINVAL, "N*K = %d*%d must be in [1, max_B = %d]", N, K, c->maxB);
    if (nword < 1 || nword + 2 > LRCN_BEAM_MAXLEN) FAIL(c, LRCN_EINVAL, "nword=%d outside [1,%d]", nword, LRCN_BEAM_MAXLEN - 2);
    if (!std::isfinite(alpha) || alpha < 0.0f) FAIL(c, LRCN_EINVAL, "alpha=%g must be finite and >= 0", (double)alpha);
    const bool diverse = G != 0;
    if (diverse && K % G != 0) FAIL(c, LRCN_EINVAL, "groups G=%d must divide the beam width K=%d", G, K);
    if (diverse && (!std::isfinite(lambda) || lambda < 0.0f)) FAIL(c, LRCN_EINVAL, "lambda=%g must be finite and >= 0", (double)lambda);
    const int FC = forced ? forced->C : 0, FA = forced ? forced->A : 0, CA = FC * FA, per = K << FC;   // per: the rows of an image
    if (forced && per > 32) FAIL(c, LRCN_EINVAL, "forced words: 2^C * K = %d * %d rows per image, at most 32", 1 << FC, K);
    if (forced && (int64_t)N * per > c->maxB) FAIL(c, LRCN_EINVAL, "forced words: N * 2^C * K = %d*%d*%d exceeds max_B = %d", N, 1 << FC, K, c->maxB);
    if (forced && nword < FC) FAIL(c, LRCN_EINVAL, "forced words: nword=%d is below the number of sets C=%d", nword, FC);
    const int R = N * per, Lh = nword + 2;
    hipStream_t st = c->stream;
    int r;
    std::vector<uint32_t> bits;
    std::vector<int32_t> table;
    const lrcn_constraints none{nullptr, 0, 0, 0};
    if (forced && !cons) cons = &none;   // rule 4 and the moves ride on the constrained path
    if (cons && (r = constraints_check(c, cons, c->V, K, nword + CA, nword, bits))) return r;
    if (forced && (r = forced_check(c, forced->words, N, FC, FA, c->V, bits, table))) return r;
    if ((r = nbest_alloc(c))) return r;
    if ((diverse || forced) && !c->dv_done) DALLOC(c, c->dv_done, sizeof(int32_t) * (size_t)c->maxB);
    if (forced && !c->fc_move) {
        DALLOC(c, c->fc_move, sizeof(float) * (size_t)c->maxB * kForcedMaxWords);
        DALLOC(c, c->fc_state, sizeof(int32_t) * (size_t)c->maxB);
    }
    float *behind = nullptr;   // the word table's place in the arena
    if (cons && (r = constraints_upload(c, bits, sizeof(int32_t) * table.size(), &behind))) return r;
    if (forced && (r = forced_upload(c, table, reinterpret_cast<int32_t *>(behind)))) return r;
    const ForcedArgs fa{reinterpret_cast<const int32_t *>(behind), FC, FA, per};
    if (ens && !c->ens_mix) DALLOC(c, c->ens_mix, sizeof(float) * (size_t)c->maxB * c->ldV);
    ConstrainArgs ca{cons ? reinterpret_cast<const uint32_t *>(c->cn_arena) : nullptr, nullptr, Lh, 0, cons ? cons->min_len : 0,
                     cons ? cons->no_repeat_ngram : 0, LRCN_EOS};
    // the members of the decode: the context itself, or the ensemble's (member 0 is c)
    const int M = ens ? ens->M : 1;
    lrcn_ctx *const one_c[1] = {c};
    const float *const *const one_p[1] = {p};
    lrcn_ctx *const *mc = ens ? ens->ctx : one_c;
    const float *const *const *mp = ens ? ens->p : one_p;
    const bool f32_logits = cons || ens;   // the top-K follows the step, from f32 logits
    DecodeRoute rt[LRCN_ENSEMBLE_MAX];
    EnsembleMixArgs mix{};
    mix.M = M;
    for (int m = 0; m < M; ++m) {
        rt[m] = decode_route(mc[m], R, per);
        if (f32_logits) rt[m].smax = false;
        if ((r = decode_begin(mc[m], mp[m], feats, N, per, rt[m]))) return member_fail(c, mc[m], m, r);
        mix.z[m] = mc[m]->st_logits;
        mix.ld[m] = mc[m]->ldV;
        mix.w[m] = ens ? ens->w[m] : 1.0f;
    }
    HIPCHK(c, hipMemsetAsync(c->bs_ndone, 0, sizeof(int32_t), st));
    DiverseState ds{};
    NbestState &ns = ds.nb;
    ns.parent = c->st_parent; ns.last = c->bs_last; ns.ndone = c->bs_ndone; ns.img = c->nb_img; ns.cum = c->nb_cum;
    ns.store = c->nb_store; ns.pool = c->nb_pool;
    ns.res_tok = c->bs_res_tok; ns.res_len = c->bs_res_len; ns.res_logp = c->bs_res_p; ns.res_score = c->nb_res_score;
    ns.K = K; ns.L = Lh; ns.nword = nword; ns.eos = LRCN_EOS;
    ns.lp_max = (float)std::pow((double)(nword + 1), (double)alpha);
    ns.seq_in = c->bs_seq[0];
    ds.done = c->dv_done; ds.G = G; ds.lambda = lambda;
    ForcedState fs{};
    fs.done = c->dv_done; fs.words = fa.words; fs.move = c->fc_move; fs.C = FC; fs.A = FA;
    fs.nb = ns;
    // histories = [bos], cum 0, next input = bos, one live slot (per group; of bank 0), empty pools
    if (forced) k_forced_init(st, fs, N, LRCN_BOS);
    else if (diverse) k_diverse_init(st, ds, N, LRCN_BOS);
    else k_nbest_init(st, ns, N, LRCN_BOS);
    for (int m = 1; m < M; ++m)   // the first step's input tokens of the other members
        HIPCHK(c, hipMemcpyAsync(mc[m]->bs_last, c->bs_last, sizeof(int32_t) * R, hipMemcpyDeviceToDevice, st));
    DecodeTail tail{};   // log-probability top-K (in the logits GEMM's epilogue + merge on the record route)
    tail.kind = DecodeTail::TOPK;
    tail.K = K;
    tail.logp = true;
    tail.records = rt[0].smax;
    if (f32_logits) tail = DecodeTail{};   // LOGITS: the top-K follows the step, from st_logits
    int cur = 0;
    for (int current = 1; current <= nword + 1; ++current) {
        for (int m = 0; m < M; ++m)
            if ((r = decode_step(mc[m], mp[m], R, rt[m], current, tail))) return member_fail(c, mc[m], m, r);
        if (ens) k_ensemble_mix_rows(st, mix, ens->log_mean, R, c->V, c->ens_mix, c->ldV);
        if (f32_logits) {
            ca.hist = c->bs_seq[cur];
            ca.current = current;
            if (forced) forced_topk_rows(c, c->st_logits, c->ldV, R, c->V, K, ca, fa, c->st_prob, c->st_topi, c->st_topv, c->fc_move, c->fc_state);
            else constrained_topk_rows(c, ens ? c->ens_mix : c->st_logits, c->ldV, R, c->V, K, ca, c->st_prob, c->st_topi, c->st_topv);
        }
        ns.seq_in = c->bs_seq[cur];
        ns.seq_out = c->bs_seq[cur ^ 1];
        ns.current = current;
        ns.lp_cur = (float)std::pow((double)current, (double)alpha);
        fs.nb = ns;
        if (forced) k_forced_update(st, c->st_topi, c->st_topv, fs, N);
        else if (diverse) k_diverse_update(st, c->st_topi, c->st_topv, ds, N);
        else k_nbest_update(st, c->st_topi, c->st_topv, ns, N);
        cur ^= 1;
        for (int m = 0; m < M; ++m) {
            if (m > 0) {   // the leader's parents and next tokens: what every member's next step continues from
                HIPCHK(c, hipMemcpyAsync(mc[m]->st_parent, c->st_parent, sizeof(int32_t) * R, hipMemcpyDeviceToDevice, st));
                HIPCHK(c, hipMemcpyAsync(mc[m]->bs_last, c->bs_last, sizeof(int32_t) * R, hipMemcpyDeviceToDevice, st));
            }
            if (!rt[m].epi) follow_parents(mc[m], R);
        }
        bool done = false;   // every image finished early?
        if ((current & 3) == 0 && current <= nword && (r = decode_poll_done(c, N, done))) return r;
        if (done) break;
    }
    KCHK(c, forced ? "beam_forced_batch" : ens ? "beam_ensemble_batch" : cons ? "beam_constrained_batch" : diverse ? "beam_diverse_batch" : "beam_nbest_batch");
    if (forced) return forced_results_to_host(c, N, K, per, Lh, out_tokens, out_len, out_logp, out_score);
    return decode_results_to_host(c, c->bs_res_tok, c->bs_res_len, c->bs_res_p, R, Lh, out_tokens, out_len, out_logp, c->nb_res_score, out_score);
}

int lrcn_beam_nbest_batch(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int K, int nword, float alpha, int32_t *out_tokens,
                          int *out_len, float *out_logp, float *out_score) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    return pool_beam_impl(c, p, feats, N, K, 0, 0.0f, nword, alpha, out_tokens, out_len, out_logp, out_score);
}

int lrcn_beam_diverse_batch(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int K, int G, float lambda, int nword, float alpha,
                            int32_t *out_tokens, int *out_len, float *out_logp, float *out_score) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (G < 1) FAIL(c, LRCN_EINVAL, "groups G=%d must be >= 1", G);
    return pool_beam_impl(c, p, feats, N, K, G, lambda, nword, alpha, out_tokens, out_len, out_logp, out_score);
}

// include/lrcn_constrain.h.  An empty set is the unconstrained call itself.
int lrcn_beam_constrained_batch(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int K, int G, float lambda, int nword, float alpha,
                                const lrcn_constraints *cons, int32_t *out_tokens, int *out_len, float *out_logp, float *out_score) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (G < 0) FAIL(c, LRCN_EINVAL, "groups G=%d must be >= 0 (0: the n-best beam)", G);
    if (cons && cons->nbanned == 0 && cons->min_len == 0 && cons->no_repeat_ngram == 0) cons = nullptr;   // (a negative field is not empty: rejected below)
    return pool_beam_impl(c, p, feats, N, K, G, G ? lambda : 0.0f, nword, alpha, out_tokens, out_len, out_logp, out_score, cons);
}

// ---------------------------------------------------------------------------------- ensembles (include/lrcn_ensemble.h, ensemble.hip)
// M, the weights (NULL: uniform; normalised in double, then rounded, into w) and the mode of both entry points
static int ensemble_check(lrcn_ctx *c, int M, const float *weights, int mode, float w[LRCN_ENSEMBLE_MAX]) {
    if (M < 1 || M > LRCN_ENSEMBLE_MAX) FAIL(c, LRCN_EINVAL, "ensemble: M=%d members outside [1, %d]", M, LRCN_ENSEMBLE_MAX);
    if (mode != LRCN_ENSEMBLE_PROB && mode != LRCN_ENSEMBLE_LOGPROB)
        FAIL(c, LRCN_EINVAL, "ensemble: mode=%d is neither LRCN_ENSEMBLE_PROB (0) nor LRCN_ENSEMBLE_LOGPROB (1)", mode);
    double sum = 0.0;
    for (int m = 0; m < M; ++m) {
        if (weights && !(std::isfinite(weights[m]) && weights[m] > 0.0f))
            FAIL(c, LRCN_EINVAL, "ensemble: the weight of member %d = %g must be positive and finite", m, (double)weights[m]);
        sum += weights ? (double)weights[m] : 1.0;
    }
    for (int m = 0; m < M; ++m) w[m] = (float)((weights ? (double)weights[m] : 1.0) / sum);
    return LRCN_OK;
}

int lrcn_beam_ensemble_batch(lrcn_ctx *const ctx[], const float *const *params[], int M, const float *weights, int mode, const float *feats, int N,
                             int K, int G, float lambda, int nword, float alpha, const lrcn_constraints *cons, int32_t *out_tokens, int *out_len,
                             float *out_logp, float *out_score) {
    if (!ctx || !ctx[0]) return LRCN_EINVAL;
    lrcn_ctx *c = ctx[0];
    DeviceGuard dg(c);
    Ensemble ens{};
    int r = ensemble_check(c, M, weights, mode, ens.w);
    if (r) return r;
    if (!params) FAIL(c, LRCN_EINVAL, "null argument");
    for (int m = 0; m < M; ++m) {
        if (!ctx[m] || !params[m]) FAIL(c, LRCN_EINVAL, "ensemble member %d: null context or parameter set", m);
        for (int q = 0; q < m; ++q)
            if (ctx[q] == ctx[m]) FAIL(c, LRCN_EINVAL, "ensemble member %d: the context of member %d (every member needs its own)", m, q);
        if (ctx[m]->V != c->V) FAIL(c, LRCN_EINVAL, "ensemble member %d: V=%d, member 0 has V=%d", m, ctx[m]->V, c->V);
        if (ctx[m]->cfg.device != c->cfg.device)
            FAIL(c, LRCN_EINVAL, "ensemble member %d: device %d, member 0 is on device %d", m, ctx[m]->cfg.device, c->cfg.device);
        if (ctx[m]->stream != c->stream) FAIL(c, LRCN_EINVAL, "ensemble member %d: its stream is not member 0's", m);
        if (N >= 1 && K >= 1 && (int64_t)N * K > ctx[m]->maxB)
            FAIL(c, LRCN_EINVAL, "ensemble member %d: N*K = %d*%d exceeds its max_B = %d", m, N, K, ctx[m]->maxB);
    }
    if (M == 1) return lrcn_beam_constrained_batch(c, params[0], feats, N, K, G, lambda, nword, alpha, cons, out_tokens, out_len, out_logp, out_score);
    if (G < 0) FAIL(c, LRCN_EINVAL, "groups G=%d must be >= 0 (0: the n-best beam)", G);
    if (cons && cons->nbanned == 0 && cons->min_len == 0 && cons->no_repeat_ngram == 0) cons = nullptr;
    ens.M = M;
    ens.ctx = ctx;
    ens.p = params;
    ens.log_mean = mode == LRCN_ENSEMBLE_LOGPROB;
    return pool_beam_impl(c, params[0], feats, N, K, G, G ? lambda : 0.0f, nword, alpha, out_tokens, out_len, out_logp, out_score, cons, &ens);
}

int lrcn_ensemble_mix_logits(lrcn_ctx *c, const float *const logits[], const int64_t ld[], int M, const float *weights, int mode, int R, int V,
                             float *out, int64_t ld_out) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    EnsembleMixArgs a{};
    int r = ensemble_check(c, M, weights, mode, a.w);
    if (r) return r;
    if (!logits || !ld || !out) FAIL(c, LRCN_EINVAL, "null argument");
    if (R < 1 || V < 1 || ld_out < V) FAIL(c, LRCN_EINVAL, "R=%d, V=%d must be >= 1 and ld_out=%lld >= V", R, V, (long long)ld_out);
    for (int m = 0; m < M; ++m) {
        if (!logits[m]) FAIL(c, LRCN_EINVAL, "ensemble member %d: null logits", m);
        if (ld[m] < V) FAIL(c, LRCN_EINVAL, "ensemble member %d: ld=%lld below V=%d", m, (long long)ld[m], V);
        a.z[m] = logits[m];
        a.ld[m] = ld[m];
    }
    a.M = M;
    k_ensemble_mix_rows(c->stream, a, mode == LRCN_ENSEMBLE_LOGPROB, R, V, out, ld_out);
    KCHK(c, "ensemble_mix_logits");
    return LRCN_OK;
}

int lrcn_constrained_topk_logits(lrcn_ctx *c, const float *logits, int64_t ld, int R, int V, int K, const lrcn_constraints *cons, const int32_t *hist,
                                 int64_t ld_hist, int current, int32_t *out_idx, float *out_logp) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (!logits || !hist || !out_idx || !out_logp) FAIL(c, LRCN_EINVAL, "null argument");
    if (R < 1 || V < 1 || ld < V || (ld & 3)) FAIL(c, LRCN_EINVAL, "R=%d, V=%d must be >= 1, ld=%lld >= V and a multiple of 4", R, V, (long long)ld);
    if (K < 1 || K > 32 || K > V) FAIL(c, LRCN_EINVAL, "K=%d must be in [1, min(32, V=%d)]", K, V);
    if (current < 1 || current > ld_hist || current > LRCN_BEAM_MAXLEN - 1)
        FAIL(c, LRCN_EINVAL, "current=%d outside [1, min(ld_hist=%lld, %d)]", current, (long long)ld_hist, LRCN_BEAM_MAXLEN - 1);
    const lrcn_constraints none{nullptr, 0, 0, 0};
    if (!cons) cons = &none;
    const bool empty = cons->nbanned == 0 && cons->min_len == 0 && cons->no_repeat_ngram == 0;   // then K <= V is all it takes
    std::vector<uint32_t> bits;
    int r = constraints_check(c, cons, V, empty ? 0 : K, current - 1, -1, bits);
    if (r) return r;
    const bool general = V > 16384 || (reinterpret_cast<uintptr_t>(logits) & 15);
    float *scratch = nullptr;
    if ((r = constraints_upload(c, bits, general ? sizeof(float) * (size_t)R * ld : 0, &scratch))) return r;
    const ConstrainArgs ca{reinterpret_cast<const uint32_t *>(c->cn_arena), hist, ld_hist, current, cons->min_len, cons->no_repeat_ngram, LRCN_EOS};
    constrained_topk_rows(c, logits, ld, R, V, K, ca, scratch, out_idx, out_logp);
    KCHK(c, "constrained_topk_logits");
    return LRCN_OK;
}

// include/lrcn_forced.h.  No sets: the constrained call itself.
int lrcn_beam_forced_batch(lrcn_ctx *c, const float *const p[9], const float *feats, int N, int K, int nword, float alpha,
                           const lrcn_constraints *cons, const lrcn_forced *forced, int32_t *out_tokens, int *out_len, float *out_logp,
                           float *out_score) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (!forced || forced->C == 0) return lrcn_beam_constrained_batch(c, p, feats, N, K, 0, 0.0f, nword, alpha, cons, out_tokens, out_len, out_logp, out_score);
    if (forced->C < 0 || forced->C > LRCN_FORCED_MAXSETS || forced->A < 1 || forced->A > LRCN_FORCED_MAXALT)
        FAIL(c, LRCN_EINVAL, "forced words: C=%d outside [0, %d] or A=%d outside [1, %d]", forced->C, LRCN_FORCED_MAXSETS, forced->A, LRCN_FORCED_MAXALT);
    if (!forced->words) FAIL(c, LRCN_EINVAL, "forced words: C=%d with a NULL table", forced->C);
    return pool_beam_impl(c, p, feats, N, K, 0, 0.0f, nword, alpha, out_tokens, out_len, out_logp, out_score, cons, nullptr, forced);
}

int lrcn_forced_topk_logits(lrcn_ctx *c, const float *logits, int64_t ld, int R, int V, int K, const lrcn_constraints *cons, const int32_t *words,
                            int C, int A, const int32_t *hist, int64_t ld_hist, int current, int32_t *out_idx, float *out_logp, float *out_move_logp,
                            int32_t *out_state) {
    if (!c) return LRCN_EINVAL;
    DeviceGuard dg(c);
    if (!logits || !hist || !out_idx || !out_logp || !out_state) FAIL(c, LRCN_EINVAL, "null argument");
    if (C < 0 || C > LRCN_FORCED_MAXSETS || (C > 0 && (A < 1 || A > LRCN_FORCED_MAXALT)))
        FAIL(c, LRCN_EINVAL, "forced words: C=%d outside [0, %d] or A=%d outside [1, %d]", C, LRCN_FORCED_MAXSETS, A, LRCN_FORCED_MAXALT);
    if (C > 0 && (!words || !out_move_logp)) FAIL(c, LRCN_EINVAL, "forced words: C=%d with a NULL table or a NULL out_move_logp", C);
    if (R < 1 || V < 1 || ld < V || (ld & 3)) FAIL(c, LRCN_EINVAL, "R=%d, V=%d must be >= 1, ld=%lld >= V and a multiple of 4", R, V, (long long)ld);
    if (K < 1 || K > 32 || K > V) FAIL(c, LRCN_EINVAL, "K=%d must be in [1, min(32, V=%d)]", K, V);
    if (current < 1 || current > ld_hist || current > LRCN_BEAM_MAXLEN - 1)
        FAIL(c, LRCN_EINVAL, "current=%d outside [1, min(ld_hist=%lld, %d)]", current, (long long)ld_hist, LRCN_BEAM_MAXLEN - 1);
    const lrcn_constraints none{nullptr, 0, 0, 0};
    if (!cons) cons = &none;
    const int FA = C > 0 ? A : 1, CA = C * FA;
    std::vector<uint32_t> bits;
    std::vector<int32_t> table;
    int r = constraints_check(c, cons, V, K, current - 1 + CA, -1, bits);
    if (r || (r = forced_check(c, words, R, C, FA, V, bits, table))) return r;
    const bool general = V > 16384 || (reinterpret_cast<uintptr_t>(logits) & 15);
    const size_t b_tab = (sizeof(int32_t) * table.size() + 255) & ~(size_t)255;
    float *behind = nullptr;
    if ((r = constraints_upload(c, bits, b_tab + (general ? sizeof(float) * (size_t)R * ld : 0), &behind))) return r;
    if ((r = forced_upload(c, table, reinterpret_cast<int32_t *>(behind)))) return r;
    const ConstrainArgs ca{reinterpret_cast<const uint32_t *>(c->cn_arena), hist, ld_hist, current, cons->min_len, cons->no_repeat_ngram, LRCN_EOS};
    const ForcedArgs fa{reinterpret_cast<const int32_t *>(behind), C, FA, 1};
    forced_topk_rows(c, logits, ld, R, V, K, ca, fa, behind + b_tab / sizeof(float), out_idx, out_logp, out_move_logp, out_state);
    KCHK(c, "forced_topk_logits");
    return LRCN_OK;
}

// Caption scoring (include/lrcn_score.h; paper section 5.1 / Table 2 -- not in lrcn.jl): see score_impl
int lrcn_score_matrix(lrcn_ctx *c, const float *const p[9], const float *feats, int N, const int32_t *tokens, const int *lens, int M, int Tmax,
                      float *scores) {
    return score_impl(c, p, feats, N, tokens, lens, M, Tmax, nullptr, nullptr, 0, scores);
}
int lrcn_score_pairs(lrcn_ctx *c, const float *const p[9], const float *feats, int N, const int32_t *tokens, const int *lens, int M, int Tmax,
                     const int32_t *pair_img, const int32_t *pair_cap, int P, float *scores) {
    if (!pair_img || !pair_cap) {
        if (c) c->err = "null argument";
        return LRCN_EINVAL;
    }
    return score_impl(c, p, feats, N, tokens, lens, M, Tmax, pair_img, pair_cap, P, scores);
}

}  // extern "C"
