// update.hip -- what turns gradients into the next step's weights: the shadow weights of the f32 parameters (DESIGN.md "shadow weights";
// two sets under LRCN_OPT_FUSED_UPDATE), update! (Adam: whole model, one gradient group, one flat run; plain, or fused with the next
// step's shadow pass) and the clipping of the global gradient norm (include/lrcn_clip.h).
#include "ctx.h"
#include "../../include/lrcn_clip.h"

using namespace lrcn_impl;

namespace {

// the 14 training shadows as an array, in a fixed order (lrcn_ctx::alt mirrors it)
struct ShadowSet {
    void *W1x, *W1h, *W1xT, *W1hT, *W2x, *W2h, *W2xT, *W2hT, *Wpd, *WpT, *Wcd, *WeT, *Wod, *WoT;
};
ShadowSet cur_shadows(const lrcn_ctx *c) {
    return ShadowSet{c->W1x, c->W1h, c->W1xT, c->W1hT, c->W2x, c->W2h, c->W2xT, c->W2hT, c->Wpd, c->WpT, c->Wcd, c->WeT, c->Wod, c->WoT};
}
ShadowSet alt_shadows(const lrcn_ctx *c) {
    void *const *a = c->alt;
    return ShadowSet{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], a[12], a[13]};
}
void swap_shadow_sets(lrcn_ctx *c) {
    void **cur[14] = {&c->W1x, &c->W1h, &c->W1xT, &c->W1hT, &c->W2x, &c->W2h, &c->W2xT, &c->W2hT, &c->Wpd, &c->WpT, &c->Wcd, &c->WeT, &c->Wod, &c->WoT};
    for (int i = 0; i < 14; ++i) std::swap(*cur[i], c->alt[i]);
    if (c->alt_gi[0]) {
        std::swap(c->W1h_gi, c->alt_gi[0]);
        std::swap(c->W2h_gi, c->alt_gi[1]);
    }
}
}  // namespace

int lrcn_impl::ensure_alt_shadows(lrcn_ctx *c) {
    if (c->alt[0]) return LRCN_OK;
    const size_t es = c->esz;
    const int H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    const size_t bytes[14] = {es * 4 * H1 * c->ldX1, es * 4 * H1 * c->ldH1, es * X1 * c->ld4H1, es * H1 * c->ld4H1,
                              es * 4 * H2 * c->ldH2, es * 4 * H2 * c->ldH2, es * H2 * c->ld4H2, es * H2 * c->ld4H2,
                              es * h * c->ldH1, es * H1 * c->ldh, es * h * LRCN_CNNOUT, es * V * c->ldE, es * V * c->ldH2, es * H2 * c->ldV};
    for (int i = 0; i < 14; ++i) DALLOC(c, c->alt[i], bytes[i]);  // zero-filled: the K padding must hold zeros
    return LRCN_OK;
}

namespace {

// the gate-interleaved recurrent weights of BOTH sets (the cell-epilogue route of a training step under LRCN_OPT_FUSED_UPDATE)
int ensure_gi_sets(lrcn_ctx *c) {
    const bool two = c->nl == 2;
    if (!c->W1h_gi) DALLOC(c, c->W1h_gi, c->esz * 4 * c->H1 * c->ldH1);
    if (two && !c->W2h_gi) DALLOC(c, c->W2h_gi, c->esz * 4 * c->H2 * c->ldH2);
    if (c->opt_fused) {
        if (!c->alt_gi[0]) DALLOC(c, c->alt_gi[0], c->esz * 4 * c->H1 * c->ldH1);
        if (two && !c->alt_gi[1]) DALLOC(c, c->alt_gi[1], c->esz * 4 * c->H2 * c->ldH2);
    }
    return LRCN_OK;
}

// the six parameter matrices of the model -> descriptors of their shadows in `w` (memory images: see the comments per line)
void plan_matrices(const lrcn_ctx *c, const float *const p[9], const ShadowSet &w, bool b, PrepPlan &plan, int only_a = -1, int only_b = -1,
                   void *const *gi = nullptr) {   // gi: {W1h, W2h} destinations with (unit, gate)-interleaved rows, or NULL
    const int E = c->E, H1 = c->H1, H2 = c->H2, h = c->h, V = c->V, X1 = c->X1;
    const bool two = c->nl == 2;
    auto add = [&](int k, int R, int C, int cs, void *dA, int64_t ldA, void *dB, int64_t ldB, void *tA, int64_t ldtA, void *tB, int64_t ldtB) {
        if (only_a >= 0 && k != only_a && k != only_b) return;
        PrepDesc &d = plan.d[plan.n++];
        d = PrepDesc{};
        d.src = p[k]; d.R = R; d.C = C; d.cs = cs;
        d.dA = dA; d.ldA = ldA; d.dB = dB; d.ldB = ldB;
        d.tA = tA; d.ldtA = ldtA; d.tB = tB; d.ldtB = ldtB;
    };
    // W1: memory [4H1][X1 + H1] -> W1x | W1h (and their transposes [X1][ld4H1] | [H1][ld4H1] for the backward dX GEMMs)
    auto with_gi = [&](int k, void *dst, int64_t ld, int H) {   // the descriptor just added (if `only` kept it) also writes the interleaved copy
        if (!dst || (only_a >= 0 && k != only_a && k != only_b)) return;
        PrepDesc &d = plan.d[plan.n - 1];
        d.dG = dst; d.ldG = ld; d.giH = H;
    };
    add(0, 4 * H1, X1 + H1, X1, w.W1x, c->ldX1, w.W1h, c->ldH1, b ? w.W1xT : nullptr, c->ld4H1, b ? w.W1hT : nullptr, c->ld4H1);
    with_gi(0, gi ? gi[0] : nullptr, c->ldH1, H1);
    if (two) {
        add(2, 4 * H2, 2 * H2, H2, w.W2x, c->ldH2, w.W2h, c->ldH2, b ? w.W2xT : nullptr, c->ld4H2, b ? w.W2hT : nullptr, c->ld4H2);
        with_gi(2, gi ? gi[1] : nullptr, c->ldH2, H2);
        add(4, h, H1, H1, w.Wpd, c->ldH1, nullptr, 0, b ? w.WpT : nullptr, c->ldh, nullptr, 0);  // Wproj (H1 x h): memory [h][H1]
    }
    add(5, h, LRCN_CNNOUT, LRCN_CNNOUT, w.Wcd, LRCN_CNNOUT, nullptr, 0, nullptr, 0, nullptr, 0);   // Wcnn: memory [h][4096]
    add(6, E, V, V, nullptr, 0, nullptr, 0, w.WeT, c->ldE, nullptr, 0);                          // Wembed (V x E): memory [E][V] -> [V][ldE]
    add(7, V, H2, H2, w.Wod, c->ldH2, nullptr, 0, b ? w.WoT : nullptr, c->ldV, nullptr, 0);   // Wout (H2 x V): memory [V][H2]
}

// update! (lrcn.jl:394) of the tensors of gradient group `group` (-1: all nine) fused with the NEXT step's shadow pass (LRCN_OPT_FUSED_UPDATE):
// the kernel writes the not-current shadow set; the caller swaps the sets once every group has been issued.
int adam_fused(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group, int step, float lr,
               float b1, float b2, float eps, hipStream_t st, const ClipCtl *clip = nullptr) {
    int r = ensure_alt_shadows(c);
    if (r) return r;
    int64_t sz[9];
    ctx_sizes(c, sz);
    PrepPlan plan{};
    const int ka = group < 0 ? -1 : kGradGroup[group][0], kb = group < 0 ? -1 : kGradGroup[group][1];
    if (c->gi_live && (r = ensure_gi_sets(c))) return r;
    plan_matrices(c, p, alt_shadows(c), true, plan, ka, kb, c->gi_live ? c->alt_gi : nullptr);
    for (int i = 0; i < plan.n; ++i) {
        PrepDesc &d = plan.d[i];
        int k = 0;
        while (k < 9 && p[k] != d.src) ++k;
        d.g = g[k]; d.m = m[k]; d.v = v[k];
    }
    for (int k : {1, 3, 8}) {  // the biases: plain Adam, one "row" of n elements
        if (sz[k] == 0 || (group >= 0 && k != ka && k != kb)) continue;
        PrepDesc &d = plan.d[plan.n++];
        d = PrepDesc{};
        d.src = p[k]; d.g = g[k]; d.m = m[k]; d.v = v[k];
        d.R = 1; d.C = (int)sz[k]; d.cs = (int)sz[k];
    }
    // (a group's update on its own stream runs beside the rest of the backward pass on an UNCAPPED grid: the groups' updates are on the step's
    // critical path, not beside it)
    plan.clip = clip;  // non-NULL: the clipped form; a skipped step still writes this set, from the unchanged parameters
    k_adam_shadows(st, c->dt, plan, step, lr, b1, b2, eps);
    KCHK(c, "adam (fused with the shadow pass)");
    return LRCN_OK;
}
void fused_update_done(lrcn_ctx *c, float *const p[9]) {  // every tensor's Adam has been issued: the written set becomes the current one
    swap_shadow_sets(c);
    for (int k = 0; k < 9; ++k) c->shadow_p[k] = p[k];
    c->shadow_valid = true;
    c->shadow_has_gi = c->gi_live && c->alt_gi[0] != nullptr;
}

// ---- include/lrcn_clip.h: the control block ----
int ensure_clip(lrcn_ctx *c) {
    if (c->clip_ctl) return LRCN_OK;
    double *parts = nullptr;
    ClipCtl *ctl = nullptr;
    DALLOC(c, parts, sizeof(double) * LRCN_CLIP_SLOTS * kSumsqParts);
    DALLOC(c, ctl, sizeof(ClipCtl));
    ClipCtl init{};
    init.scale = 1.0f;  // an update that reads the block before any lrcn_clip_set is the plain update
    HIPCHK(c, hipMemcpy(ctl, &init, sizeof(init), hipMemcpyHostToDevice));
    c->clip_parts = parts;
    c->clip_ctl = ctl;
    return LRCN_OK;
}

// the nine tensors of an update that is not fused with the shadow pass; ka >= 0: only tensors ka and kb have a length
AdamTensors adam_tensors(float *const p[9], const float *const g[9], float *const m[9], float *const v[9], const int64_t sz[9], int ka = -1,
                         int kb = -1) {
    AdamTensors t;
    for (int k = 0; k < 9; ++k) {
        t.w[k] = p[k];
        t.g[k] = g[k];
        t.m[k] = m[k];
        t.v[k] = v[k];
        t.n[k] = ka < 0 || k == ka || k == kb ? sz[k] : 0;
    }
    return t;
}

// lrcn_adam_update_flat and its clipped namesake
int adam_update_flat(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1, float b2, float eps,
                     void *stream, bool clipped) {
    DeviceGuard dg(c);
    if (!c || step < 1 || n < 0) return LRCN_EINVAL;
    if (n == 0) return LRCN_OK;
    if (!w || !g || !m || !v) return LRCN_EINVAL;
    int r = clipped ? ensure_clip(c) : LRCN_OK;  // clipped: scale and skip come from the context's control block
    if (r) return r;
    const ClipCtl *clip = clipped ? c->clip_ctl : nullptr;
    hipStream_t st = stream_or_ctx(c, stream);
    c->shadow_valid = false;  // some parameter changed: the next call makes its shadow weights afresh
    SegScope seg(c, LRCN_SEG_UPDATE, st, 28.0 * (double)n);
    AdamTensors t{};
    t.w[0] = w; t.g[0] = g; t.m[0] = m; t.v[0] = v; t.n[0] = n;
    k_adam(st, t, step, lr, b1, b2, eps, clip);
    KCHK(c, "adam (flat)");
    return LRCN_OK;
}

}  // namespace

// f32 column-major params -> K-contiguous shadows in T (direct and transposed).  See DESIGN.md "shadow weights".
int lrcn_impl::prepare_weights(lrcn_ctx *c, const float *const p[9], const ShadowNeed &need) {
    const int dt = c->dt, H1 = c->H1, H2 = c->H2, X1 = c->X1;
    if (!p[0] || !p[1] || !p[5] || !p[6] || !p[7] || !p[8] || (c->nl == 2 && (!p[2] || !p[3] || !p[4]))) FAIL(c, LRCN_EINVAL, "null parameter tensor");
    hipStream_t st = c->stream;
    const bool two = c->nl == 2;
    // LRCN_OPT_FUSED_UPDATE: the previous train step's Adam kernel already wrote this set from these very parameters
    if (need.gi || need.dec_tables) {
        int rg = ensure_gi_sets(c);
        if (rg) return rg;
        if (need.gi) c->gi_live = true;   // from now on the fused update writes the interleaved copies with the other shadows
    }
    const bool gi = need.gi || need.dec_tables;   // (dec_tables makes the interleaved copies without making them sticky)
    if (c->opt_fused && c->shadow_valid && !need.cat && (!gi || c->shadow_has_gi)) {
        bool same = true;
        for (int k = 0; k < 9; ++k) same = same && c->shadow_p[k] == p[k];
        if (same) return LRCN_OK;
    }
    c->shadow_valid = false;
    c->refresh_groups = 0;  // a full shadow pass supersedes a per-group refresh sequence that was left unfinished
    PrepPlan plan{};
    void *const gi_cur[2] = {c->W1h_gi, c->W2h_gi};
    plan_matrices(c, p, cur_shadows(c), need.bwd, plan, -1, -1, gi ? gi_cur : nullptr);
    if (need.dec_tables && c->nl == 2) {
        // W2 (memory [4H2][2 H2]: columns [h1 Wproj (h) | x_cnn (h) | h2 (H2)]) -> dec_W2c [4H2][ldh + ldH2] = [proj columns | h2 columns], rows
        // (unit, gate)-interleaved: two descriptors over the same source, each with one live side
        const int64_t ld = c->ldh + c->ldH2;
        PrepDesc &a = plan.d[plan.n++];
        a = PrepDesc{};
        a.src = p[2]; a.R = 4 * H2; a.C = 2 * H2; a.cs = c->h; a.dA = c->dec_W2c; a.ldA = ld; a.permH = H2;
        PrepDesc &b = plan.d[plan.n++];
        b = PrepDesc{};
        b.src = p[2]; b.R = 4 * H2; b.C = 2 * H2; b.cs = H2; b.dB = boff(c->dec_W2c, c->ldh, c->esz); b.ldB = ld; b.permH = H2;
    }
    if (need.cat) {  // batched decode: W1 / W2 with the x and h column blocks each padded to whole K-steps, side by side
        // cat_perm: the rows in (unit, gate)-interleaved order, for the decode step with the cell math in the GEMM's epilogue
        auto add = [&](const float *src, int R, int C, int cs, void *dA, int64_t ldA, void *dB, int64_t ldB, int permH) {
            PrepDesc &d = plan.d[plan.n++];
            d = PrepDesc{};
            d.src = src; d.R = R; d.C = C; d.cs = cs; d.dA = dA; d.ldA = ldA; d.dB = dB; d.ldB = ldB;
            d.permH = need.cat_perm ? permH : 0;
        };
        add(p[0], 4 * H1, X1 + H1, X1, c->W1cat, c->ldXH1, boff(c->W1cat, c->ldX1, c->esz), c->ldXH1, H1);
        if (two) add(p[2], 4 * H2, 2 * H2, H2, c->W2cat, c->ldXH2, boff(c->W2cat, c->ldH2, c->esz), c->ldXH2, H2);
    }
    k_prepare_weights(st, dt, plan);
    KCHK(c, "prepare_weights");
    return LRCN_OK;
}

int lrcn_impl::adam_update(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step, float lr,
                           float b1, float b2, float eps, bool clipped) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || step < 1) return LRCN_EINVAL;
    int r = clipped ? ensure_clip(c) : LRCN_OK;  // clipped: scale and skip come from the context's control block
    if (r) return r;
    const ClipCtl *clip = clipped ? c->clip_ctl : nullptr;
    c->fused_groups = 0;  // the whole-model update supersedes any per-group sequence left unfinished (an error between two groups)
    int64_t sz[9], nparam = 0;
    ctx_sizes(c, sz);
    for (int k = 0; k < 9; ++k) nparam += sz[k];
    SegScope seg(c, LRCN_SEG_UPDATE, c->stream, 28.0 * (double)nparam);  // w, m, v read + written, g read: 28 B per parameter
    c->shadow_valid = false;
    if (c->opt_fused) {  // LRCN_OPT_FUSED_UPDATE: the same update, and the next step's shadow weights in the same pass
        r = adam_fused(c, p, g, m, v, -1, step, lr, b1, b2, eps, c->stream, clip);
        if (r) return r;
        fused_update_done(c, p);
        return LRCN_OK;
    }
    k_adam(c->stream, adam_tensors(p, g, m, v, sz), step, lr, b1, b2, eps, clip);
    KCHK(c, "adam");
    return LRCN_OK;
}

int lrcn_impl::adam_update_group(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                                 int step, float lr, float b1, float b2, float eps, void *stream, bool clipped) {
    DeviceGuard dg(c);
    if (!c || !p || !g || !m || !v || step < 1) return LRCN_EINVAL;
    if (group < 0 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [0,%d)", group, LRCN_GRAD_GROUPS);
    int r = clipped ? ensure_clip(c) : LRCN_OK;  // clipped: scale and skip come from the context's control block
    if (r) return r;
    const ClipCtl *clip = clipped ? c->clip_ctl : nullptr;
    const int ka = kGradGroup[group][0], kb = kGradGroup[group][1];
    hipStream_t st = stream_or_ctx(c, stream);
    int64_t sz[9];
    ctx_sizes(c, sz);
    SegScope seg(c, LRCN_SEG_UPDATE, st, 28.0 * (double)(sz[ka] + (kb != ka ? sz[kb] : 0)));
    c->shadow_valid = false;
    if (c->opt_fused) {
        // fused with the shadow pass; the written set becomes current once all five groups of this step have been issued (they are
        // issued in any order, each exactly once per step, with the same `step`)
        if (step != c->fused_step) {  // first group of a new step: bits left by a step that never completed do not count
            c->fused_groups = 0;
            c->fused_step = step;
        }
        r = adam_fused(c, p, g, m, v, group, step, lr, b1, b2, eps, st, clip);
        if (r) {
            c->fused_groups = 0;
            return r;
        }
        c->fused_groups |= 1u << group;
        if (c->fused_groups == (1u << LRCN_GRAD_GROUPS) - 1) {
            c->fused_groups = 0;
            fused_update_done(c, p);
        }
        return LRCN_OK;
    }
    k_adam(st, adam_tensors(p, g, m, v, sz, ka, kb), step, lr, b1, b2, eps, clip);
    KCHK(c, "adam (group)");
    return LRCN_OK;
}

extern "C" {

int lrcn_adam_update(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step,
                     float lr, float b1, float b2, float eps) {
    return adam_update(c, p, g, m, v, step, lr, b1, b2, eps, false);
}

int lrcn_adam_update_group(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                           int step, float lr, float b1, float b2, float eps, void *stream) {
    return adam_update_group(c, p, g, m, v, group, step, lr, b1, b2, eps, stream, false);
}

int lrcn_adam_update_flat(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1, float b2,
                          float eps, void *stream) {
    return adam_update_flat(c, w, g, m, v, n, step, lr, b1, b2, eps, stream, false);
}

int lrcn_refresh_shadows_group(lrcn_ctx *c, const float *const p[9], int group, void *stream) {
    DeviceGuard dg(c);
    if (!c || !p) return LRCN_EINVAL;
    if (group < 0 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [0,%d)", group, LRCN_GRAD_GROUPS);
    if (!c->opt_fused) FAIL(c, LRCN_ESTATE, "lrcn_refresh_shadows_group needs LRCN_OPT_FUSED_UPDATE = 1 (the second shadow set)");
    int r = ensure_alt_shadows(c);
    if (r) return r;
    if (c->refresh_groups == 0) c->shadow_valid = false;  // first group of a step: the current set describes the OLD parameters from now on
    PrepPlan plan{};
    if (c->gi_live && (r = ensure_gi_sets(c))) return r;
    plan_matrices(c, p, alt_shadows(c), true, plan, kGradGroup[group][0], kGradGroup[group][1], c->gi_live ? c->alt_gi : nullptr);
    if (plan.n > 0) {  // LRCN-1f has no W2 / Wproj: an empty group is only counted
        k_prepare_weights(stream_or_ctx(c, stream), c->dt, plan);
        KCHK(c, "refresh_shadows_group");
    }
    c->refresh_groups |= 1u << group;
    if (c->refresh_groups == (1u << LRCN_GRAD_GROUPS) - 1) {
        c->refresh_groups = 0;
        float *pp[9];
        for (int k = 0; k < 9; ++k) pp[k] = const_cast<float *>(p[k]);
        fused_update_done(c, pp);
    }
    return LRCN_OK;
}

// ---- include/lrcn_clip.h: global gradient-norm clipping ----
int lrcn_grad_sumsq(lrcn_ctx *c, const float *g, int64_t n, int slot, void *stream) {
    DeviceGuard dg(c);
    if (!c || n < 0 || (!g && n > 0)) return LRCN_EINVAL;
    if (slot < 0 || slot >= LRCN_CLIP_SLOTS) FAIL(c, LRCN_EINVAL, "slot=%d outside [0,%d)", slot, LRCN_CLIP_SLOTS);
    int r = ensure_clip(c);
    if (r) return r;
    SumsqArgs a{};
    a.g[0] = g; a.n[0] = n; a.slot[0] = slot; a.count = 1;
    k_sumsq(stream_or_ctx(c, stream), a, c->clip_parts, c->clip_ctl);
    KCHK(c, "sumsq");
    return LRCN_OK;
}

int lrcn_grad_sumsq_model(lrcn_ctx *c, const float *const g[9], int group, void *stream) {
    DeviceGuard dg(c);
    if (!c || !g) return LRCN_EINVAL;
    if (group < -1 || group >= LRCN_GRAD_GROUPS) FAIL(c, LRCN_EINVAL, "group=%d outside [-1,%d)", group, LRCN_GRAD_GROUPS);
    int64_t sz[9];
    ctx_sizes(c, sz);
    SumsqArgs a{};
    for (int k = 0; k < 9; ++k) {
        if (group >= 0 && k != kGradGroup[group][0] && k != kGradGroup[group][1]) continue;
        if (sz[k] > 0 && !g[k]) return LRCN_EINVAL;
        a.g[a.count] = g[k]; a.n[a.count] = sz[k]; a.slot[a.count] = k;
        ++a.count;
    }
    int r = ensure_clip(c);
    if (r) return r;
    k_sumsq(stream_or_ctx(c, stream), a, c->clip_parts, c->clip_ctl);
    KCHK(c, "sumsq (model)");
    return LRCN_OK;
}

int lrcn_clip_slots(lrcn_ctx *c, double **dev_ptr) {
    DeviceGuard dg(c);
    if (!c || !dev_ptr) return LRCN_EINVAL;
    int r = ensure_clip(c);
    if (r) return r;
    *dev_ptr = c->clip_ctl->slot;  // (address arithmetic only: the block is never read from the host here)
    return LRCN_OK;
}

int lrcn_clip_set(lrcn_ctx *c, int n_slots, float max_norm, void *stream) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (n_slots < 1 || n_slots > LRCN_CLIP_SLOTS) FAIL(c, LRCN_EINVAL, "n_slots=%d outside [1,%d]", n_slots, LRCN_CLIP_SLOTS);
    if (!(max_norm > 0.0f)) FAIL(c, LRCN_EINVAL, "max_norm=%g is not > 0", (double)max_norm);
    int r = ensure_clip(c);
    if (r) return r;
    k_clip_set(stream_or_ctx(c, stream), c->clip_ctl, n_slots, max_norm);
    KCHK(c, "clip_set");
    return LRCN_OK;
}

int lrcn_adam_update_clipped(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int step,
                             float lr, float b1, float b2, float eps) {
    return adam_update(c, p, g, m, v, step, lr, b1, b2, eps, true);
}

int lrcn_adam_update_group_clipped(lrcn_ctx *c, float *const p[9], const float *const g[9], float *const m[9], float *const v[9], int group,
                                   int step, float lr, float b1, float b2, float eps, void *stream) {
    return adam_update_group(c, p, g, m, v, group, step, lr, b1, b2, eps, stream, true);
}

int lrcn_adam_update_flat_clipped(lrcn_ctx *c, float *w, const float *g, float *m, float *v, int64_t n, int step, float lr, float b1,
                                  float b2, float eps, void *stream) {
    return adam_update_flat(c, w, g, m, v, n, step, lr, b1, b2, eps, stream, true);
}

int lrcn_clip_stats(lrcn_ctx *c, lrcn_clip_stats_t *out) {
    DeviceGuard dg(c);
    if (!c || !out) return LRCN_EINVAL;
    int r = ensure_clip(c);
    if (r) return r;
    ClipCtl h{};
    HIPCHK(c, hipMemcpyAsync(&h, c->clip_ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out->last_norm = h.norm;
    out->last_scale = h.scale;
    out->last_skipped = h.skip;
    out->steps = h.steps;
    out->clipped = h.clipped;
    out->skipped = h.skipped;
    return LRCN_OK;
}

}  // extern "C"
