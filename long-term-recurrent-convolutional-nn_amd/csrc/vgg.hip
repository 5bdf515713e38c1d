// vgg.hip -- the VGG-16 forward of the caption model (include/lrcn.h): convolution layers, vgg_body, the VGG and image-front entry points,
// the upload ring of lrcn_upload_crops, the single-layer convolution entry points and the convolution / GEMM bench helpers.
#include <algorithm>
#include <cstring>

#include "ctx.h"
#include "../../include/lrcn_conv_debug.h"
#include "../../include/lrcn_gemm_debug.h"

using namespace lrcn_impl;

// ------------------------------------------------------------------------------------------- VGG
static const int kVggCout[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int kVggPool[13] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1};

namespace {
// kernel development (LRCN_STAMPS, lrcn_debug_stamps): c->stamps grown to at least `need` stamps; the previous, smaller buffer stays on the
// context's allocation list until lrcn_destroy
int stamps_reserve(lrcn_ctx *c, int64_t need) {
    if (need > c->stamps_n) {
        c->stamps = nullptr;
        DALLOC(c, c->stamps, sizeof(unsigned long long) * (size_t)need);
        c->stamps_n = need;
    }
    return LRCN_OK;
}
bool conv64_enabled() { return !knob_off("LRCN_CONV64"); }  // LRCN_CONV64=0 routes the Cin = 64 layers back to the implicit-GEMM kernels
// f8_inv_scale > 0: write e4m3(out * f8_inv_scale) if the layer's kernel can (returns *wrote_f8), else bf16 as usual
constexpr int kTileCtrStride = 8 + 2 * 512;  // ints per layer: 8 queue heads + two hand-off slots per workgroup (<= 512 workgroups)
// An implicit-GEMM convolution of N images (g.M = N * H * W rows, operands and output of `es` bytes per element), cut into launches
// of whole images whose input stays below the 4 GiB that the direct-to-LDS kernels address with 32-bit offsets (bf16 conv2_2 from
// 1171 images, conv3_1 from 5349; images are independent, so the cut costs nothing but the tail of one more launch).
// Without it a larger batch fell through to the register-staged kernel: 2048 images 72.8 ms per forward, 28 k images/s.
hipError_t launch_conv_chunked(hipStream_t st, const GemmArgs &g0, int N, int es, int64_t limit_bytes = 0) {
    const int64_t per_img = (int64_t)g0.H * g0.W * g0.Cin * es;
    // limit_bytes: LRCN_OPT_CONV_CHUNK_BYTES (tests force several chunks at a handful of images; at least one image per launch)
    int64_t cap = ((limit_bytes > 0 ? limit_bytes : 0xF0000000ll) - (limit_bytes > 0 ? 0 : (int64_t)(g0.W + 1) * g0.Cin * es)) / per_img;
    if (limit_bytes > 0 && cap < 1) cap = 1;
    if (N <= cap || cap < 1) return launch_gemm(st, g0);
    const int nch = (int)((N + cap - 1) / cap), per = (N + nch - 1) / nch;
    const int64_t out_img = (int64_t)(g0.out_mode == GEMM_OUT_POOL ? (g0.H / 2) * (g0.W / 2) : g0.H * g0.W) * g0.ldc * es;
    for (int n0 = 0; n0 < N; n0 += per) {
        GemmArgs g = g0;
        const int n = N - n0 < per ? N - n0 : per;
        g.A = reinterpret_cast<const unsigned char *>(g0.A) + (int64_t)n0 * per_img;
        g.C = reinterpret_cast<unsigned char *>(g0.C) + (int64_t)n0 * out_img;
        g.M = n * g0.H * g0.W;
        g.tile_ctr = nullptr;  // one set of tile queues per launch
        if (hipError_t e = launch_gemm(st, g); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The implicit-GEMM descriptor of one 3x3 convolution (+ bias, relu, pool) of N images with the layer's T weights (conv_layer, conv_layer_fp8)
GemmArgs conv_args(const lrcn_ctx *c, int dtype, const void *in, const VggLayer &L, int N, void *out, int *tile_ctr) {
    GemmArgs g{};
    g.dtype = dtype;
    g.A = in;
    g.B = L.w;
    g.ldb = 9 * L.Cin;
    g.C = out;
    g.ldc = L.Cout;
    g.M = N * L.S * L.S;
    g.N = L.Cout;
    g.K = 9 * L.Cin;
    g.bias = L.b;
    g.relu = 1;
    g.a_mode = GEMM_A_CONV3;
    g.out_mode = L.pool ? GEMM_OUT_POOL : GEMM_OUT_CONV;
    g.H = g.W = L.S;
    g.Cin = L.Cin;
    g.zero_page = c->zero_page;
    g.wg_cap = c->vgg_wg_cap;
    g.tile_ctr = (c->vgg_wg_cap >= 8 && c->vgg_wg_cap <= 512) ? tile_ctr : nullptr;
    return g;
}

int conv_layer(lrcn_ctx *c, int dtype, const void *in, const VggLayer &L, int N, void *out, float f8_inv_scale = 0.0f, bool *wrote_f8 = nullptr,
               int *tile_ctr = nullptr) {
    if (wrote_f8) *wrote_f8 = false;
    if (conv64_enabled() && conv64_eligible(dtype, L.Cin, L.Cout, L.S, L.S)) {
        const bool f8 = f8_inv_scale > 0.0f && !L.pool;
        if (wrote_f8) *wrote_f8 = f8;
        unsigned long long *stamps = nullptr;
        if (knob_set("LRCN_STAMPS")) {  // kernel development (tools/conv64_stamps.py): 16 stamps per 16 x 16 tile per 64-channel chunk 0
            if (int r = stamps_reserve(c, (int64_t)N * (L.S / 16) * (L.S / 16) * 16)) return r;
            stamps = c->stamps;
        }
        hipError_t e = launch_conv64(c->stream, in, L.w, L.b, out, N, L.S, L.S, L.Cout, 1, L.pool, c->zero_page, f8 ? f8_inv_scale : 0.0f, c->vgg_wg_cap, stamps);
        if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv64 layer S=%d Cout=%d: %s", L.S, L.Cout, hipGetErrorString(e));
        return LRCN_OK;
    }
    GemmArgs g = conv_args(c, dtype, in, L, N, out, tile_ctr);
    g.ws = c->vgg_ws;  // one split-K workspace per stream: the VGG forward may run beside the LSTM step (gemm_ws)
    g.ws_bytes = c->vgg_ws ? c->gemm_ws_bytes : 0;
    if (knob_set("LRCN_STAMPS")) {  // kernel-development (include/lrcn.h lrcn_debug_stamps)
        if (int r = stamps_reserve(c, ((int64_t)g.M / 256 + 1) * ((int64_t)g.N / 128 + 1) * 8)) return r;
        g.stamps = c->stamps;
    }
    hipError_t e = launch_conv_chunked(c->stream, g, N, dtype == GEMM_T_BF16 ? 2 : 4, c->conv_chunk_bytes);
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv layer S=%d Cin=%d Cout=%d: %s", L.S, L.Cin, L.Cout, hipGetErrorString(e));
    return LRCN_OK;
}

// e4m3 in -> e4m3 out (lrcn.jl:724-728 conv4 .+ b, relu, pool at reduced precision; scales from lrcn_vgg_calibrate)
int conv_layer_fp8(lrcn_ctx *c, const void *in, const VggLayer &L, int N, void *out, int *tile_ctr = nullptr) {
    GemmArgs g = conv_args(c, GEMM_T_F8, in, L, N, out, tile_ctr);
    g.B = L.w8;
    g.bias = L.ebias;
    g.scale = L.escale;
    // the e4m3 kernel addresses its A operand with SIGNED 32-bit element offsets (gemm_8p_f8_ok: M * Cin < 2^31), half of what the bf16 / f32
    // descriptors reach: cut at 2 GiB minus a margin (round 6: 1536 and 2048 images failed at conv2_2 -- 3.3 GB of e4m3 input in one launch)
    hipError_t e = launch_conv_chunked(c->stream, g, N, 1, c->conv_chunk_bytes > 0 ? c->conv_chunk_bytes : 0x7F000000ll);
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "fp8 conv layer S=%d Cin=%d Cout=%d: %s", L.S, L.Cin, L.Cout, hipGetErrorString(e));
    return LRCN_OK;
}

}  // namespace

namespace lrcn_impl {

// source image (uint8 crops or the preprocessed float tensor) -> featsRM [N][4096] f32
// calibrate: run every layer in bf16 and collect the output amax of conv2_1 .. conv5_3 (post-pool) into amax_dev
int vgg_body(lrcn_ctx *c, int N, const void *src, bool src_u8, const float *mean, bool calibrate) {
    const bool fp8 = c->vgg_fp8 && !calibrate;
    if (fp8 && !c->fp8_ready) FAIL(c, LRCN_ESTATE, "vgg_dtype = LRCN_FP8: call lrcn_vgg_calibrate before the first forward");
    const int vdt = c->vdt;
    const float m0 = mean ? mean[0] : 0.f, m1 = mean ? mean[1] : 0.f, m2 = mean ? mean[2] : 0.f;
    // LRCN_FUSE11=0: conv1_1 and conv1_2 as two launches
    const bool fuse11 = vdt == GEMM_T_BF16 && src_u8 && c->conv[0].w_fused && conv64_enabled() && !knob_off("LRCN_FUSE11");
    const float *avg = (src_u8 && c->avg_on) ? c->avg_img : nullptr;
    // crops that arrived through lrcn_upload_crops: the forward's stream waits for the upload; the staging buffer is free again as soon as the
    // ONE kernel below that reads the uint8 source has run (recorded right after it)
    int staged = -1;
    if (src_u8)
        for (int j = 0; j < lrcn_ctx::kStage; ++j)
            if (c->stage[j] && src == c->stage[j]) staged = j;
    if (staged >= 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->up_done[staged], 0));
    auto crops_consumed = [&]() -> int {
        if (staged < 0) return LRCN_OK;
        HIPCHK(c, hipEventRecord(c->rd_done[staged], c->stream));
        c->stage_read[staged] = true;
        c->stage_full[staged] = false;
        staged = -1;
        return LRCN_OK;
    };
    if (avg && !fuse11) {
        // full averageImage outside the fused path: read_image_data's arithmetic as its own pass into a float tensor (lrcn.jl:770-771),
        // then the float-input route
        if (!c->pre_f32) DALLOC(c, c->pre_f32, sizeof(float) * (size_t)c->cfg.max_images * 224 * 224 * 3);
        k_preprocess_u8(c->stream, reinterpret_cast<const uint8_t *>(src), N, 224, 0.f, 0.f, 0.f, avg, c->pre_f32);
        if (int r = crops_consumed()) return r;
        src = c->pre_f32;
        src_u8 = false;
    }
    c->vgg_routes.clear();
    auto note = [&](const char *r) {
        if (!c->vgg_routes.empty()) c->vgg_routes += ',';
        c->vgg_routes += r;
    };
    if (fuse11) {
        // read_image_data's arithmetic as an elementwise pass (38 MB -> 77 MB at N = 256); conv1_1 itself runs inside conv1_2's launch
        SegScope seg_pp(c, LRCN_SEG_PREPROCESS, c->stream, 3.0 * N * 224 * 224 * 3);  // 1 B in, one bf16 out per pixel value
        k_img_u8_to_bf16(c->stream, reinterpret_cast<const uint8_t *>(src), (int64_t)N * 224 * 224 * 3, m0, m1, m2, avg, 224, c->img16);
    } else if (vdt == GEMM_T_BF16) {
        // conv1_1 fused with the preprocessing arithmetic (conv11.hip): HBM-bound, no im2col in memory
        k_conv11_fused(c->stream, src_u8 ? 1 : 0, src, N, 224, m0, m1, m2, c->conv[0].w, c->conv[0].b, c->actA);
    } else {
        // f32: conv1_1 as a plain GEMM over an explicit im2col (K = 27), scattered to NHWC
        if (src_u8)
            k_im2col11_u8(c->stream, vdt, reinterpret_cast<const uint8_t *>(src), N, 224, m0, m1, m2, c->im2col, 32);
        else
            k_im2col11_f32(c->stream, vdt, reinterpret_cast<const float *>(src), N, 224, c->im2col, 32);
        GemmArgs g{};
        g.dtype = vdt;
        g.A = c->im2col;
        g.lda = 32;
        g.B = c->conv[0].w;
        g.ldb = 32;
        g.C = c->actA;
        g.ldc = 64;
        g.M = N * 224 * 224;
        g.N = 64;
        g.K = 27;
        g.bias = c->conv[0].b;
        g.relu = 1;
        g.a_mode = GEMM_A_PLAIN;
        g.out_mode = GEMM_OUT_CONV;
        g.H = g.W = 224;
        g.zero_page = c->zero_page;
        hipError_t e = launch_gemm(c->stream, g);
        if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv1_1: %s", hipGetErrorString(e));
    }
    // (f32: the im2col pass above was the reader and the GEMM after it does not touch the crops -- recording behind it only delays the release)
    if (int r = crops_consumed()) return r;
    if (!fuse11) note(vdt == GEMM_T_BF16 ? "conv11" : gemm_debug_last_route());
    void *cur = c->actA, *nxt = c->actB;
    // capped persistent grids (the two-stream training step): LRCN_DYN_TILES=1 makes the workgroups of a layer PULL their tiles
    // from per-XCD queues instead of walking static round-robin shares.  Measured and left off: the hypothesis was that a
    // workgroup starting late (its CU still held by an LSTM-stream kernel) stretches the whole launch; pulling costs 2 % alone
    // (6.59 -> 6.74 ms per forward at cap 224) and gains nothing in the step (7.54 -> 7.64 ms) -- the contention is not tail imbalance.
    int *ctr = nullptr;
    if (c->vgg_wg_cap >= 8 && knob_char("LRCN_DYN_TILES") == '1') {
        if (!c->tile_ctr) DALLOC(c, c->tile_ctr, sizeof(int) * 13 * kTileCtrStride);
        HIPCHK(c, hipMemsetAsync(c->tile_ctr, 0, sizeof(int) * 13 * kTileCtrStride, c->stream));
        ctr = c->tile_ctr;
    }
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    if (c->prof) {
        if (c->prof_used == c->prof_ev.size()) {
            std::pair<hipEvent_t, hipEvent_t> e;
            HIPCHK(c, hipEventCreate(&e.first));
            HIPCHK(c, hipEventCreate(&e.second));
            c->prof_ev.push_back(e);
        }
        ev = &c->prof_ev[c->prof_used++];
        HIPCHK(c, hipEventRecord(ev->first, c->stream));
    }
    int l0 = 1;
    if (fuse11) {  // conv1_1 + conv1_2 + pool1 in one launch, straight from the uint8 crops: actA is never written
        unsigned long long *stamps = nullptr;
        if (knob_char("LRCN_STAMPS") == 'f') {  // LRCN_STAMPS=f: stamp the fused conv1 kernel of a VGG forward
            if (int r = stamps_reserve(c, (int64_t)N * 14 * 14 * 16)) return r;
            stamps = c->stamps;
        }
        hipError_t e = launch_conv64_fused11(c->stream, c->img16, c->conv[0].w_fused, c->conv[0].b, c->conv[1].w, c->conv[1].b, nxt, N, 224,
                                             c->zero_page, c->vgg_wg_cap, stamps);
        if (e != hipSuccess) FAIL(c, LRCN_EHIP, "fused conv1_1+conv1_2: %s", hipGetErrorString(e));
        note(gemm_debug_last_route());
        std::swap(cur, nxt);
        l0 = 2;
    }
    auto out_count = [&](int l) {
        const VggLayer &L = c->conv[l];
        const int64_t So = L.pool ? L.S / 2 : L.S;
        return (int64_t)N * So * So * L.Cout;
    };
    bool in_is_f8 = false;
    for (int l = l0; l < 13; ++l) {
        if (fp8 && l == kFp8First && !in_is_f8) {  // conv2_1 ran on a kernel without the e4m3 epilogue: one elementwise pass
            k_cast_bf16_fp8(c->stream, cur, out_count(l - 1), 1.0f / c->act_scale[l - 1], nxt);
            std::swap(cur, nxt);
        }
        int r;
        if (fp8 && l >= kFp8First)
            r = conv_layer_fp8(c, cur, c->conv[l], N, nxt, ctr ? ctr + l * kTileCtrStride : nullptr);
        else  // conv2_1 writes the e4m3 input of conv2_2 directly when it runs on conv64.hip
            r = conv_layer(c, vdt, cur, c->conv[l], N, nxt, (fp8 && l == kFp8First - 1) ? 1.0f / c->act_scale[l] : 0.0f, &in_is_f8,
                           ctr ? ctr + l * kTileCtrStride : nullptr);
        if (r) return r;
        note(gemm_debug_last_route());
        std::swap(cur, nxt);
        if (calibrate && l >= kFp8First - 1) k_amax(c->stream, cur, out_count(l), c->amax_dev + l);
    }
    if (fp8) {  // pool5 e4m3 -> bf16 for fc6
        k_cast_fp8_bf16(c->stream, cur, out_count(12), c->act_scale[12], nxt);
        std::swap(cur, nxt);
    }
    if (ev) HIPCHK(c, hipEventRecord(ev->second, c->stream));
    // cur = pool5 output [N][7*7*512]; fc6 + relu6; fc7 (no relu7: lrcn.jl:717)
    GemmArgs g{};
    g.dtype = vdt;
    g.A = cur;
    g.lda = 25088;
    g.B = c->fc6w;
    g.ldb = 25088;
    g.M = N;
    g.N = 4096;
    g.K = 25088;
    g.zero_page = c->zero_page;
    g.ws = c->vgg_ws;
    g.ws_bytes = c->gemm_ws_bytes;
    g.C = c->f6;
    g.ldc = 4096;
    g.bias = c->fc6b;
    g.relu = 1;
    hipError_t e = launch_gemm(c->stream, g);  // N = 256 images: 205 MB of weights through 32 tiles -> gemm_8p's split-K form
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "fc6: %s", hipGetErrorString(e));
    note(gemm_debug_last_route());
    g.A = c->f6;
    g.lda = 4096;
    g.B = c->fc7w;
    g.ldb = 4096;
    g.C = c->featsRM;
    g.K = 4096;
    g.bias = c->fc7b;
    g.relu = 0;
    g.c_f32 = 1;
    e = launch_gemm(c->stream, g);
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "fc7: %s", hipGetErrorString(e));
    note(gemm_debug_last_route());
    return LRCN_OK;
}
int vgg_check(lrcn_ctx *c, int N) {
    if (!c->vgg_loaded) FAIL(c, LRCN_ESTATE, "lrcn_vgg_load has not been called");
    if (N < 1 || N > c->cfg.max_images) FAIL(c, LRCN_EINVAL, "N=%d outside [1,%d]", N, c->cfg.max_images);
    return LRCN_OK;
}
}  // namespace lrcn_impl

extern "C" {

int lrcn_vgg_load(lrcn_ctx *c, const float *const cw[13], const float *const cb[13], const float *fc6_w, const float *fc6_b,
                  const float *fc7_w, const float *fc7_b) {
    DeviceGuard dg(c);
    if (!c || !cw || !cb || !fc6_w || !fc6_b || !fc7_w || !fc7_b) return LRCN_EINVAL;
    if (c->cfg.max_images < 1) FAIL(c, LRCN_ESTATE, "context was created with max_images = 0");
    if (c->vgg_loaded) FAIL(c, LRCN_ESTATE, "VGG weights already loaded");
    const int vdt = c->vdt;
    const size_t ve = c->vesz;
    hipStream_t st = c->stream;
    int Cin = 3, S = 224;
    for (int l = 0; l < 13; ++l) {
        VggLayer &L = c->conv[l];
        L.Cin = Cin;
        L.Cout = kVggCout[l];
        L.S = S;
        L.pool = kVggPool[l];
        DALLOC(c, L.b, sizeof(float) * L.Cout);
        HIPCHK(c, hipMemcpyAsync(L.b, cb[l], sizeof(float) * L.Cout, hipMemcpyDeviceToDevice, st));
        if (l == 0) {
            DALLOC(c, L.w, ve * 64 * 32);
            k_repack_conv11_w(st, vdt, cw[0], 64, L.w, 32);
            if (vdt == GEMM_T_BF16) {
                DALLOC(c, L.w_fused, 2 * 64 * 32);
                k_repack_conv11_w_fused(st, cw[0], cb[0], L.w_fused);
            }
        } else {
            DALLOC(c, L.w, ve * (size_t)L.Cout * 9 * Cin);
            k_repack_conv_w(st, vdt, cw[l], Cin, L.Cout, Cin, L.w);
            if (c->vgg_fp8 && l >= kFp8First) {
                DALLOC(c, L.w8, (size_t)L.Cout * 9 * Cin);
                DALLOC(c, L.sw, sizeof(float) * L.Cout);
                DALLOC(c, L.escale, sizeof(float) * L.Cout);
                DALLOC(c, L.ebias, sizeof(float) * L.Cout);
                k_quant_conv_w_fp8(st, cw[l], Cin, L.Cout, L.w8, L.sw);
            }
        }
        Cin = L.Cout;
        if (L.pool) S /= 2;
    }
    DALLOC(c, c->fc6w, ve * 4096ull * 25088ull);
    DALLOC(c, c->fc7w, ve * 4096ull * 4096ull);
    DALLOC(c, c->fc6b, sizeof(float) * 4096);
    DALLOC(c, c->fc7b, sizeof(float) * 4096);
    k_repack_fc6_w(st, vdt, fc6_w, c->fc6w);
    k_transpose(st, vdt, 1, fc7_w, 4096, 4096, 4096, c->fc7w, 4096, 0);  // (o,k) at o + 4096k -> [o][k]
    HIPCHK(c, hipMemcpyAsync(c->fc6b, fc6_b, sizeof(float) * 4096, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->fc7b, fc7_b, sizeof(float) * 4096, hipMemcpyDeviceToDevice, st));
    KCHK(c, "vgg_load");
    HIPCHK(c, hipStreamSynchronize(st));
    c->vgg_loaded = true;
    return LRCN_OK;
}

// Diagnostic: time one bf16 implicit-GEMM convolution layer (random data) in isolation: avg ms over `iters` launches.
int lrcn_bench_conv(lrcn_ctx *c, int N, int S, int Cin, int Cout, int pool, int iters, double *ms_out) {
    DeviceGuard dg(c);
    if (!c || !ms_out || N < 1 || S < 2 || (S & 1) || Cin % 64 || Cout < 1 || iters < 1) return LRCN_EINVAL;
    const size_t in_e = (size_t)N * S * S * Cin, w_e = (size_t)Cout * 9 * Cin, out_e = (size_t)N * S * S * Cout;
    void *in = nullptr, *w = nullptr, *out = nullptr;
    float *tmp = nullptr, *bias = nullptr;
    hipEvent_t e0, e1;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(in); (void)hipFree(w); (void)hipFree(out); (void)hipFree(tmp); (void)hipFree(bias);
    };
    const size_t big = in_e > w_e ? in_e : w_e;
    if (hipMalloc(&in, 2 * in_e) != hipSuccess || hipMalloc(&w, 2 * w_e) != hipSuccess || hipMalloc(&out, 2 * out_e) != hipSuccess ||
        hipMalloc((void **)&tmp, 4 * big) != hipSuccess || hipMalloc((void **)&bias, 4 * Cout) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "bench_conv scratch");
    }
    k_init_uniform(c->stream, tmp, (int64_t)in_e, 1.0f, 11, 0);
    // cast in row chunks of Cin (k_cast_rows works row-wise)
    k_cast_rows(c->stream, GEMM_T_BF16, tmp, Cin, (int)(in_e / Cin), Cin, in, Cin);
    k_init_uniform(c->stream, tmp, (int64_t)w_e, (float)std::sqrt(2.0 / (9.0 * Cin)), 12, 1);
    k_cast_rows(c->stream, GEMM_T_BF16, tmp, 9 * Cin, Cout, 9 * Cin, w, 9 * Cin);
    k_fill(c->stream, bias, Cout, 0.01f);
    VggLayer L;
    L.w = w; L.b = bias; L.Cin = Cin; L.Cout = Cout; L.S = S; L.pool = pool;
    int r = conv_layer(c, GEMM_T_BF16, in, L, N, out);  // warm-up
    if (r) { cleanup(); return r; }
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    for (int i = 0; i < iters && !r; ++i) r = conv_layer(c, GEMM_T_BF16, in, L, N, out);
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    cleanup();
    if (r) return r;
    *ms_out = ms / iters;
    return LRCN_OK;
}

// Diagnostic: time one bf16 NT GEMM C[M][N] = A[M][K] B[N][K]^T (random data, bf16 output) through launch_gemm.
int lrcn_bench_gemm(lrcn_ctx *c, int M, int N, int K, int iters, double *ms_out) {
    DeviceGuard dg(c);
    if (!c || !ms_out || M < 1 || N < 8 || K < 64 || (K % 64) || (N % 8) || iters < 1) return LRCN_EINVAL;
    void *A = nullptr, *B = nullptr, *C = nullptr;
    float *tmp = nullptr;
    const size_t ae = (size_t)M * K, be = (size_t)N * K, ce = (size_t)M * N;
    const size_t big = ae > be ? ae : be;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(A); (void)hipFree(B); (void)hipFree(C); (void)hipFree(tmp);
    };
    if (hipMalloc(&A, 2 * ae) != hipSuccess || hipMalloc(&B, 2 * be) != hipSuccess || hipMalloc(&C, 2 * ce) != hipSuccess ||
        hipMalloc((void **)&tmp, 4 * big) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "bench_gemm scratch");
    }
    k_init_uniform(c->stream, tmp, (int64_t)ae, 1.0f, 21, 0);
    k_cast_rows(c->stream, GEMM_T_BF16, tmp, K, M, K, A, K);
    k_init_uniform(c->stream, tmp, (int64_t)be, 1.0f, 22, 1);
    k_cast_rows(c->stream, GEMM_T_BF16, tmp, K, N, K, B, K);
    int r = gemm(c, GEMM_T_BF16, A, K, B, K, C, N, M, N, K, nullptr, false);
    if (r) { cleanup(); return r; }
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, c->stream);
    for (int i = 0; i < iters && !r; ++i) r = gemm(c, GEMM_T_BF16, A, K, B, K, C, N, M, N, K, nullptr, false);
    (void)hipEventRecord(e1, c->stream);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    cleanup();
    if (r) return r;
    *ms_out = ms / iters;
    return LRCN_OK;
}

// Test entry (include/lrcn_gemm_debug.h): ONE contraction through launch_gemm on the caller's operands, filled as lrcn_impl::gemm fills its
// own -- except K, which goes to the engines as given, and the router inputs lrcn_impl::gemm derives from a capped VGG grid, which the
// caller states.  No allocation, no conversion; the stream is drained before the call returns.
int lrcn_debug_gemm(lrcn_ctx *c, const lrcn_gemm_debug *d) {
    DeviceGuard dg(c);
    if (!c || !d) return LRCN_EINVAL;
    if (d->dtype != LRCN_F32 && d->dtype != LRCN_BF16) FAIL(c, LRCN_EINVAL, "debug_gemm: dtype %d is neither f32 nor bf16", d->dtype);
    GemmArgs g{};
    g.dtype = d->dtype == LRCN_BF16 ? GEMM_T_BF16 : GEMM_T_F32;
    g.A = d->A;
    g.lda = d->lda;
    g.B = d->B;
    g.ldb = d->ldb;
    g.C = d->C;
    g.ldc = d->ldc;
    g.M = d->M;
    g.N = d->N;
    g.K = d->K;
    g.bias = d->bias;
    g.c_f32 = d->c_f32 != 0;
    g.beta = d->beta != 0;
    g.c_is_zero = d->c_is_zero != 0;
    g.relu = d->relu != 0;
    g.a_mode = GEMM_A_PLAIN;
    g.out_mode = GEMM_OUT_PLAIN;
    g.zero_page = c->zero_page;
    g.deterministic = d->deterministic != 0;
    g.ws = c->gemm_ws;
    g.ws_bytes = c->gemm_ws_bytes;
    g.free_cus = d->free_cus;
    g.bg_cus = d->bg_cus;
    g.wg_cap = d->wg_cap;
    const hipError_t e = launch_gemm(c->stream, g);
    if (e != hipSuccess)
        FAIL(c, e == hipErrorInvalidValue ? LRCN_EINVAL : LRCN_EHIP, "debug_gemm M=%d N=%d K=%d: %s", d->M, d->N, d->K, hipGetErrorString(e));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LRCN_OK;
}

// Test entry (include/lrcn_gemm_debug.h): ONE 3x3 convolution through launch_gemm in CONV3 mode on the caller's NHWC operands, filled as
// conv_args / lrcn_conv3x3 fill theirs (static tile walk: no tile queues).  No allocation, no conversion, never conv64.hip; the stream is
// drained before the call returns.
int lrcn_debug_conv_gemm(lrcn_ctx *c, const lrcn_conv_gemm_debug *d) {
    DeviceGuard dg(c);
    if (!c || !d) return LRCN_EINVAL;
    if (d->dtype != LRCN_F32 && d->dtype != LRCN_BF16) FAIL(c, LRCN_EINVAL, "debug_conv_gemm: dtype %d is neither f32 nor bf16", d->dtype);
    if (d->N < 1 || d->H < 2 || d->W < 2 || d->Cin < 1 || d->Cout < 1 || d->ldc < d->Cout || (int64_t)d->N * d->H * d->W > 0x7FFFFFFF ||
        (int64_t)9 * d->Cin > 0x7FFFFFFF)
        FAIL(c, LRCN_EINVAL, "debug_conv_gemm: N=%d H=%d W=%d Cin=%d Cout=%d ldc=%lld", d->N, d->H, d->W, d->Cin, d->Cout, (long long)d->ldc);
    GemmArgs g{};
    g.dtype = d->dtype == LRCN_BF16 ? GEMM_T_BF16 : GEMM_T_F32;
    g.A = d->x;
    g.B = d->w;
    g.ldb = 9 * (int64_t)d->Cin;
    g.C = d->y;
    g.ldc = d->ldc;
    g.M = d->N * d->H * d->W;
    g.N = d->Cout;
    g.K = 9 * d->Cin;
    g.bias = d->bias;
    g.relu = d->relu != 0;
    g.a_mode = GEMM_A_CONV3;
    g.out_mode = d->pool ? GEMM_OUT_POOL : GEMM_OUT_CONV;
    g.H = d->H;
    g.W = d->W;
    g.Cin = d->Cin;
    g.zero_page = c->zero_page;
    g.ws = c->gemm_ws;
    g.ws_bytes = c->gemm_ws_bytes;
    g.wg_cap = d->wg_cap;
    g.tile_ctr = nullptr;
    const hipError_t e = launch_gemm(c->stream, g);
    if (e != hipSuccess)
        FAIL(c, e == hipErrorInvalidValue ? LRCN_EINVAL : LRCN_EHIP, "debug_conv_gemm N=%d H=%d W=%d Cin=%d Cout=%d: %s", d->N, d->H, d->W, d->Cin,
             d->Cout, hipGetErrorString(e));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LRCN_OK;
}

// ---- input feed (rev 4) ----
int lrcn_host_alloc(void **host_ptr, size_t bytes) {
    if (!host_ptr) return LRCN_EINVAL;
    *host_ptr = nullptr;
    return hipHostMalloc(host_ptr, bytes ? bytes : 16, hipHostMallocDefault) == hipSuccess ? LRCN_OK : LRCN_ENOMEM;
}
int lrcn_host_free(void *host_ptr) { return hipHostFree(host_ptr) == hipSuccess ? LRCN_OK : LRCN_EHIP; }

int lrcn_upload_crops(lrcn_ctx *c, const uint8_t *host_u8, int N, const uint8_t **dev_out) {
    DeviceGuard dg(c);
    if (!c || !host_u8 || !dev_out) return LRCN_EINVAL;
    *dev_out = nullptr;
    if (c->cfg.max_images < 1) FAIL(c, LRCN_ESTATE, "context was created with max_images = 0");
    if (N < 1 || N > c->cfg.max_images) FAIL(c, LRCN_EINVAL, "N=%d outside [1,%d]", N, c->cfg.max_images);
    const size_t per = (size_t)224 * 224 * 3;
    if (!c->copy_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (int j = 0; j < lrcn_ctx::kStage; ++j) {
            HIPCHK(c, hipEventCreateWithFlags(&c->up_done[j], hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&c->rd_done[j], hipEventDisableTiming));
            DALLOC(c, c->stage[j], per * (size_t)c->cfg.max_images);
        }
    }
    const int j = c->stage_next;
    if (c->stage_full[j])
        FAIL(c, LRCN_ESTATE, "all %d staging buffers hold crops that no VGG forward has been issued on yet (upload at most %d batches ahead)",
             lrcn_ctx::kStage, lrcn_ctx::kStage);
    // the forward that last read this buffer: normally long finished; otherwise wait for it HERE, on the host (see lrcn_ctx::kStage)
    if (c->stage_read[j] && hipEventQuery(c->rd_done[j]) != hipSuccess) HIPCHK(c, hipEventSynchronize(c->rd_done[j]));
    {
        SegScope seg_up(c, LRCN_SEG_UPLOAD, c->copy_stream, (double)per * N);
        HIPCHK(c, hipMemcpyAsync(c->stage[j], host_u8, per * (size_t)N, hipMemcpyHostToDevice, c->copy_stream));
    }
    HIPCHK(c, hipEventRecord(c->up_done[j], c->copy_stream));
    c->stage_full[j] = true;
    c->stage_next = (j + 1) % lrcn_ctx::kStage;
    *dev_out = c->stage[j];
    return LRCN_OK;
}

int lrcn_upload_wait(lrcn_ctx *c) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (c->copy_stream) HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    return LRCN_OK;
}

int lrcn_vgg_forward(lrcn_ctx *c, const float *x, int N, float *feats) {
    DeviceGuard dg(c);
    if (!c || !x || !feats) return LRCN_EINVAL;
    int r = vgg_check(c, N);
    if (r) return r;
    r = vgg_body(c, N, x, false, nullptr);
    if (r) return r;
    k_transpose_f32(c->stream, c->featsRM, 4096, N, 4096, feats, N);  // return transpose(xs): N x 4096 column-major
    KCHK(c, "vgg_forward");
    return LRCN_OK;
}

int lrcn_vgg_forward_u8(lrcn_ctx *c, const uint8_t *img, int N, const float mean[3], float *feats) {
    DeviceGuard dg(c);
    if (!c || !img || !feats || (!mean && !c->avg_on)) return LRCN_EINVAL;
    int r = vgg_check(c, N);
    if (r) return r;
    r = vgg_body(c, N, img, true, mean);
    if (r) return r;
    k_transpose_f32(c->stream, c->featsRM, 4096, N, 4096, feats, N);
    KCHK(c, "vgg_forward_u8");
    return LRCN_OK;
}

int lrcn_vgg_forward_u8_blocks(lrcn_ctx *c, const uint8_t *img, int N, const float mean[3], int block_rows, int normalize, float *feats) {
    DeviceGuard dg(c);
    if (!c || !img || !feats || (!mean && !c->avg_on)) return LRCN_EINVAL;
    int r = vgg_check(c, N);
    if (r) return r;
    if (block_rows < 1 || N % block_rows) FAIL(c, LRCN_EINVAL, "block_rows=%d must divide N=%d", block_rows, N);
    r = vgg_body(c, N, img, true, mean);
    if (r) return r;
    for (int b = 0; b < N / block_rows; ++b) {  // block b: rows [b block_rows, (b+1) block_rows) as its own block_rows x 4096 column-major array
        float *dst = feats + (int64_t)b * block_rows * LRCN_CNNOUT;
        k_transpose_f32(c->stream, c->featsRM + (int64_t)b * block_rows * LRCN_CNNOUT, 4096, block_rows, 4096, dst, block_rows);
        if (normalize) k_normalize_rows(c->stream, dst, block_rows, LRCN_CNNOUT);
    }
    KCHK(c, "vgg_forward_u8_blocks");
    return LRCN_OK;
}

int lrcn_preprocess_u8(lrcn_ctx *c, const uint8_t *img, int N, const float mean[3], float *out) {
    DeviceGuard dg(c);
    if (!c || !img || !out || (!mean && !c->avg_on) || N < 1) return LRCN_EINVAL;
    k_preprocess_u8(c->stream, img, N, 224, mean ? mean[0] : 0.f, mean ? mean[1] : 0.f, mean ? mean[2] : 0.f, c->avg_on ? c->avg_img : nullptr, out);
    KCHK(c, "preprocess_u8");
    return LRCN_OK;
}

int lrcn_set_average_image(lrcn_ctx *c, const float *avg) {
    DeviceGuard dg(c);
    if (!c) return LRCN_EINVAL;
    if (!avg) {
        c->avg_on = false;
        return LRCN_OK;
    }
    if (!c->avg_img) DALLOC(c, c->avg_img, sizeof(float) * 224 * 224 * 3);
    HIPCHK(c, hipMemcpyAsync(c->avg_img, avg, sizeof(float) * 224 * 224 * 3, hipMemcpyDeviceToDevice, c->stream));
    c->avg_on = true;
    return LRCN_OK;
}

int lrcn_resize_crop_u8(lrcn_ctx *c, const uint8_t *src, const int64_t *offsets, const int *heights, const int *widths, const int *channels,
                        int N, uint8_t *out) {
    DeviceGuard dg(c);
    if (!c || !src || !offsets || !heights || !widths || !channels || !out) return LRCN_EINVAL;
    if (N < 1 || N > 65536) FAIL(c, LRCN_EINVAL, "N=%d outside [1,65536]", N);
    struct Meta {
        int64_t off;
        int h, w, ch, pad;
    };
    std::vector<Meta> m(N);
    for (int n = 0; n < N; ++n) {
        if (heights[n] < 1 || widths[n] < 1 || heights[n] > 32768 || widths[n] > 32768 || (channels[n] != 1 && channels[n] != 3 && channels[n] != 4) ||
            offsets[n] < 0)
            FAIL(c, LRCN_EINVAL, "image %d: %d x %d x %d at offset %lld (need 1..32768 pixels per side, 1, 3 or 4 channels)", n, heights[n],
                 widths[n], channels[n], (long long)offsets[n]);
        m[n] = Meta{offsets[n], heights[n], widths[n], channels[n], 0};
    }
    if (N > c->img_meta_cap) {
        void *p = nullptr;
        const int cap = N < 256 ? 256 : N;
        if (hipMalloc(&p, sizeof(Meta) * (size_t)cap) != hipSuccess) FAIL(c, LRCN_ENOMEM, "image descriptors");
        c->allocs.push_back(p);  // the old (smaller) buffer stays owned by the context until lrcn_destroy
        c->img_meta = p;
        c->img_meta_cap = cap;
    }
    HIPCHK(c, hipMemcpyAsync(c->img_meta, m.data(), sizeof(Meta) * (size_t)N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // m goes out of scope
    k_resize_crop_u8(c->stream, src, c->img_meta, N, 224, out);
    KCHK(c, "resize_crop_u8");
    return LRCN_OK;
}

int lrcn_normalize_features(lrcn_ctx *c, float *feats, int N) {
    DeviceGuard dg(c);
    if (!c || !feats || N < 1) return LRCN_EINVAL;
    k_normalize_rows(c->stream, feats, N, LRCN_CNNOUT);
    KCHK(c, "normalize_features");
    return LRCN_OK;
}

int lrcn_conv3x3(lrcn_ctx *c, const float *x, int W, int H, int Cin, int N, const float *w, const float *b, int Cout, int relu,
                 int pool, float *y) {
    DeviceGuard dg(c);
    if (!c || !x || !w || !b || !y) return LRCN_EINVAL;
    if (W < 2 || H < 2 || (W & 1) || (H & 1) || Cin < 1 || Cout < 1 || N < 1) FAIL(c, LRCN_EINVAL, "conv3x3: W,H must be even, sizes positive");
    const int vdt = c->vdt;
    const size_t ve = c->vesz;
    const int bk = vdt == GEMM_T_BF16 ? 64 : 32;
    const int Cp = (int)round_up64(Cin, bk);
    void *xin = nullptr, *wp = nullptr, *out = nullptr;
    float *bd = nullptr;
    const int Wo = pool ? W / 2 : W, Ho = pool ? H / 2 : H;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(xin);
        (void)hipFree(wp);
        (void)hipFree(out);
        (void)hipFree(bd);
    };
    if (hipMalloc(&xin, ve * (size_t)N * H * W * Cp) != hipSuccess || hipMalloc(&wp, ve * (size_t)Cout * 9 * Cp) != hipSuccess ||
        hipMalloc(&out, ve * (size_t)N * Ho * Wo * Cout) != hipSuccess || hipMalloc((void **)&bd, sizeof(float) * Cout) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "conv3x3 scratch");
    }
    (void)hipMemcpyAsync(bd, b, sizeof(float) * Cout, hipMemcpyDeviceToDevice, c->stream);
    k_ref_to_nhwc(c->stream, vdt, x, W, H, Cin, N, xin, Cp);
    k_repack_conv_w(c->stream, vdt, w, Cin, Cout, Cp, wp);
    if (conv64_enabled() && conv64_eligible(vdt, Cp, Cout, H, W)) {
        hipError_t e = launch_conv64(c->stream, xin, wp, bd, out, N, H, W, Cout, relu, pool, c->zero_page);
        if (e == hipSuccess) {
            k_nhwc_to_ref(c->stream, vdt, out, Wo, Ho, Cout, N, Cout, y);
            e = hipGetLastError();
        }
        cleanup();
        if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv3x3 (conv64): %s", hipGetErrorString(e));
        return LRCN_OK;
    }
    GemmArgs g{};
    g.dtype = vdt;
    g.A = xin;
    g.B = wp;
    g.ldb = 9 * Cp;
    g.C = out;
    g.ldc = Cout;
    g.M = N * H * W;
    g.N = Cout;
    g.K = 9 * Cp;
    g.bias = bd;
    g.relu = relu;
    g.a_mode = GEMM_A_CONV3;
    g.out_mode = pool ? GEMM_OUT_POOL : GEMM_OUT_CONV;
    g.H = H;
    g.W = W;
    g.Cin = Cp;
    g.zero_page = c->zero_page;
    g.ws = c->gemm_ws;
    g.ws_bytes = c->gemm_ws_bytes;
    hipError_t e = launch_gemm(c->stream, g);
    if (e == hipSuccess) {
        k_nhwc_to_ref(c->stream, vdt, out, Wo, Ho, Cout, N, Cout, y);
        e = hipGetLastError();
    }
    cleanup();
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv3x3: %s", hipGetErrorString(e));
    return LRCN_OK;
}

int lrcn_conv1_fused(lrcn_ctx *c, const uint8_t *img, int N, int S, const float mean[3], const float *w11, const float *b11, const float *w12,
                     const float *b12, float *y) {
    DeviceGuard dg(c);
    if (!c || !img || !mean || !w11 || !b11 || !w12 || !b12 || !y) return LRCN_EINVAL;
    if (N < 1 || S < 16 || (S % 16) || (int64_t)N * (S + 4) * (S + 4) * 3 >= (1ll << 31)) FAIL(c, LRCN_EINVAL, "conv1_fused: S must be a multiple of 16, N >= 1");
    void *img16 = nullptr, *wf = nullptr, *wp = nullptr, *out = nullptr;
    float *bd = nullptr;
    const int So = S / 2;
    const size_t img16_bytes = 2 * ((size_t)N * (S + 4) * (S + 4) * 3 + 8);
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(img16);
        (void)hipFree(wf);
        (void)hipFree(wp);
        (void)hipFree(out);
        (void)hipFree(bd);
    };
    if (hipMalloc(&img16, img16_bytes) != hipSuccess || hipMalloc(&wf, 2 * 64 * 32) != hipSuccess || hipMalloc(&wp, 2 * (size_t)64 * 9 * 64) != hipSuccess ||
        hipMalloc(&out, 2 * (size_t)N * So * So * 64) != hipSuccess || hipMalloc((void **)&bd, sizeof(float) * 128) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "conv1_fused scratch");
    }
    (void)hipMemsetAsync(img16, 0, img16_bytes, c->stream);  // the 2-pixel frame is conv1_1's zero padding
    (void)hipMemcpyAsync(bd, b11, sizeof(float) * 64, hipMemcpyDeviceToDevice, c->stream);
    (void)hipMemcpyAsync(bd + 64, b12, sizeof(float) * 64, hipMemcpyDeviceToDevice, c->stream);
    k_img_u8_to_bf16(c->stream, img, (int64_t)N * S * S * 3, mean[0], mean[1], mean[2], nullptr, S, img16);
    k_repack_conv11_w_fused(c->stream, w11, bd, wf);
    k_repack_conv_w(c->stream, GEMM_T_BF16, w12, 64, 64, 64, wp);
    hipError_t e = launch_conv64_fused11(c->stream, img16, wf, bd, wp, bd + 64, out, N, S, c->zero_page, c->vgg_wg_cap);
    if (e == hipSuccess) {
        k_nhwc_to_ref(c->stream, GEMM_T_BF16, out, So, So, 64, N, 64, y);
        e = hipGetLastError();
    }
    cleanup();
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv1_fused: %s", hipGetErrorString(e));
    return LRCN_OK;
}

// Test entry (include/lrcn_conv_debug.h): conv11.hip's kernel by itself on the caller's source, weights repacked as lrcn_vgg_load repacks them
int lrcn_debug_conv11(lrcn_ctx *c, const void *src, int src_is_u8, int N, int S, const float mean[3], const float *w11, const float *b11,
                      float *y) {
    DeviceGuard dg(c);
    if (!c || !src || (src_is_u8 && !mean) || !w11 || !b11 || !y) return LRCN_EINVAL;
    if (c->vdt != GEMM_T_BF16) FAIL(c, LRCN_EINVAL, "debug_conv11: the context's vgg_dtype must be LRCN_BF16 or LRCN_FP8");
    if (N < 1 || S < 2 || (S & 1) || (int64_t)N * S * S * 64 >= (1ll << 31)) FAIL(c, LRCN_EINVAL, "debug_conv11: S must be even and >= 2, N >= 1");
    void *wp = nullptr, *out = nullptr;
    float *bd = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(wp);
        (void)hipFree(out);
        (void)hipFree(bd);
    };
    if (hipMalloc(&wp, 2 * 64 * 32) != hipSuccess || hipMalloc(&out, 2 * (size_t)N * S * S * 64) != hipSuccess ||
        hipMalloc((void **)&bd, sizeof(float) * 64) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "debug_conv11 scratch");
    }
    (void)hipMemcpyAsync(bd, b11, sizeof(float) * 64, hipMemcpyDeviceToDevice, c->stream);
    k_repack_conv11_w(c->stream, GEMM_T_BF16, w11, 64, wp, 32);
    k_conv11_fused(c->stream, src_is_u8 ? 1 : 0, src, N, S, src_is_u8 ? mean[0] : 0.f, src_is_u8 ? mean[1] : 0.f, src_is_u8 ? mean[2] : 0.f, wp,
                   bd, out);
    k_nhwc_to_ref(c->stream, GEMM_T_BF16, out, S, S, 64, N, 64, y);
    const hipError_t e = hipGetLastError();
    cleanup();
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "debug_conv11: %s", hipGetErrorString(e));
    return LRCN_OK;
}

// Test entries of the fp8 stack's seams (include/lrcn_conv_debug.h)
int lrcn_debug_fp8_cast(lrcn_ctx *c, int dir, const void *src, int64_t n, float factor, void *dst) {
    DeviceGuard dg(c);
    if (!c || !src || !dst) return LRCN_EINVAL;
    if (c->vdt != GEMM_T_BF16) FAIL(c, LRCN_EINVAL, "debug_fp8_cast: the context's vgg_dtype must be LRCN_BF16 or LRCN_FP8");
    if (n < 8 || n % 8 || (reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(dst) & 15))
        FAIL(c, LRCN_EINVAL, "debug_fp8_cast: n=%lld must be a positive multiple of 8, both buffers 16-byte aligned", (long long)n);
    if (!(factor > 0.0f) || !std::isfinite(factor)) FAIL(c, LRCN_EINVAL, "debug_fp8_cast: factor=%g must be finite and positive", factor);
    if (dir == 0)
        k_cast_bf16_fp8(c->stream, src, n, factor, dst);
    else
        k_cast_fp8_bf16(c->stream, src, n, factor, dst);
    KCHK(c, "debug_fp8_cast");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LRCN_OK;
}

int lrcn_debug_amax(lrcn_ctx *c, const void *x_bf16, int64_t n, float *out_dev) {
    DeviceGuard dg(c);
    if (!c || !x_bf16 || !out_dev) return LRCN_EINVAL;
    if (n < 1) FAIL(c, LRCN_EINVAL, "debug_amax: n=%lld < 1", (long long)n);
    HIPCHK(c, hipMemsetAsync(out_dev, 0, sizeof(float), c->stream));
    k_amax(c->stream, x_bf16, n, out_dev);
    KCHK(c, "debug_amax");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LRCN_OK;
}

int lrcn_debug_conv64_f8(lrcn_ctx *c, const float *x, int W, int H, int N, const float *w, const float *b, int Cout, float f8_inv_scale,
                         float *y) {
    DeviceGuard dg(c);
    if (!c || !x || !w || !b || !y) return LRCN_EINVAL;
    if (c->vdt != GEMM_T_BF16) FAIL(c, LRCN_EINVAL, "debug_conv64_f8: the context's vgg_dtype must be LRCN_BF16 or LRCN_FP8");
    if (N < 1 || !conv64_eligible(GEMM_T_BF16, 64, Cout, H, W) || (int64_t)N * H * W * 64 >= (1ll << 31))
        FAIL(c, LRCN_EINVAL, "debug_conv64_f8: W, H multiples of 16, Cout a multiple of 64, N >= 1, N*W*H*64 < 2^31");
    if (!(f8_inv_scale > 0.0f) || !std::isfinite(f8_inv_scale))
        FAIL(c, LRCN_EINVAL, "debug_conv64_f8: f8_inv_scale=%g must be finite and positive", f8_inv_scale);
    void *xin = nullptr, *wp = nullptr, *out = nullptr;
    float *bd = nullptr;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(xin);
        (void)hipFree(wp);
        (void)hipFree(out);
        (void)hipFree(bd);
    };
    if (hipMalloc(&xin, 2 * (size_t)N * H * W * 64) != hipSuccess || hipMalloc(&wp, 2 * (size_t)Cout * 9 * 64) != hipSuccess ||
        hipMalloc(&out, (size_t)N * H * W * Cout) != hipSuccess || hipMalloc((void **)&bd, sizeof(float) * Cout) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "debug_conv64_f8 scratch");
    }
    (void)hipMemcpyAsync(bd, b, sizeof(float) * Cout, hipMemcpyDeviceToDevice, c->stream);
    k_ref_to_nhwc(c->stream, GEMM_T_BF16, x, W, H, 64, N, xin, 64);
    k_repack_conv_w(c->stream, GEMM_T_BF16, w, 64, Cout, 64, wp);
    hipError_t e = launch_conv64(c->stream, xin, wp, bd, out, N, H, W, Cout, 1, 0, c->zero_page, f8_inv_scale, c->vgg_wg_cap);
    if (e == hipSuccess) {
        k_nhwc_fp8_to_ref(c->stream, out, W, H, Cout, N, 1.0f, y);
        e = hipGetLastError();
    }
    cleanup();
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "debug_conv64_f8: %s", hipGetErrorString(e));
    return LRCN_OK;
}

// Test entry (include/lrcn_conv_debug.h): conv64.hip's plain kernel on the caller's NHWC bf16 operands under the caller's workgroup cap.
// No allocation, no conversion; every refusal happens here, before launch_conv64 is called; the stream is drained before the call returns.
int lrcn_debug_conv64(lrcn_ctx *c, const lrcn_conv64_debug *d) {
    DeviceGuard dg(c);
    if (!c || !d) return LRCN_EINVAL;
    if (!d->x || !d->w || !d->y) FAIL(c, LRCN_EINVAL, "debug_conv64: x, w and y must not be NULL");
    if (c->vdt != GEMM_T_BF16) FAIL(c, LRCN_EINVAL, "debug_conv64: the context's vgg_dtype must be LRCN_BF16 or LRCN_FP8");
    if (d->N < 1 || !conv64_eligible(GEMM_T_BF16, 64, d->Cout, d->H, d->W) || (int64_t)d->N * d->H * d->W * 64 >= (1ll << 31))
        FAIL(c, LRCN_EINVAL, "debug_conv64: W, H multiples of 16, Cout a multiple of 64, N >= 1, N*W*H*64 < 2^31 (N=%d H=%d W=%d Cout=%d)", d->N, d->H,
             d->W, d->Cout);
    if ((reinterpret_cast<uintptr_t>(d->x) | reinterpret_cast<uintptr_t>(d->w) | reinterpret_cast<uintptr_t>(d->y)) & 15)
        FAIL(c, LRCN_EINVAL, "debug_conv64: x, w and y must be 16-byte aligned");
    // bias == NULL: no bias pointer goes down, and the kernel's bias stage then holds zeros
    const hipError_t e = launch_conv64(c->stream, d->x, d->w, d->bias, d->y, d->N, d->H, d->W, d->Cout, d->relu != 0, d->pool != 0, c->zero_page, 0.0f,
                                       d->wg_cap);
    if (e != hipSuccess)
        FAIL(c, e == hipErrorInvalidValue ? LRCN_EINVAL : LRCN_EHIP, "debug_conv64 N=%d H=%d W=%d Cout=%d: %s", d->N, d->H, d->W, d->Cout,
             hipGetErrorString(e));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LRCN_OK;
}

int lrcn_debug_fp8_scales(lrcn_ctx *c, float out[13]) {
    if (!c || !out) return LRCN_EINVAL;
    if (!c->vgg_fp8 || !c->fp8_ready) FAIL(c, LRCN_ESTATE, "debug_fp8_scales: needs a vgg_dtype = LRCN_FP8 context after lrcn_vgg_calibrate");
    for (int l = 0; l < 13; ++l) out[l] = l >= kFp8First - 1 ? c->act_scale[l] : 0.0f;
    return LRCN_OK;
}

int lrcn_vgg_calibrate(lrcn_ctx *c, const uint8_t *img, int N, const float mean[3], float margin) {
    DeviceGuard dg(c);
    if (!c || !img || (!mean && !c->avg_on)) return LRCN_EINVAL;
    if (!c->vgg_fp8) FAIL(c, LRCN_ESTATE, "lrcn_vgg_calibrate needs a context created with vgg_dtype = LRCN_FP8");
    if (!(margin >= 1.0f) || margin > 16.0f) FAIL(c, LRCN_EINVAL, "margin=%g outside [1,16]", margin);
    int r = vgg_check(c, N);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->amax_dev, 0, sizeof(float) * 16, c->stream));
    r = vgg_body(c, N, img, true, mean, true);
    if (r) return r;
    float amax[16];
    HIPCHK(c, hipMemcpyAsync(amax, c->amax_dev, sizeof(float) * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int l = kFp8First - 1; l < 13; ++l) {
        if (!(amax[l] > 0.0f) || !std::isfinite(amax[l])) FAIL(c, LRCN_ESTATE, "calibration: layer %d output amax = %g", l, amax[l]);
        c->act_scale[l] = margin * amax[l] / 448.0f;
    }
    for (int l = kFp8First; l < 13; ++l) {
        const VggLayer &L = c->conv[l];
        k_fp8_epilogue_params(c->stream, L.b, L.sw, L.Cout, c->act_scale[l - 1], c->act_scale[l], L.escale, L.ebias);
    }
    KCHK(c, "vgg_calibrate");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->fp8_ready = true;
    return LRCN_OK;
}

int lrcn_conv3x3_fp8(lrcn_ctx *c, const float *x, int W, int H, int Cin, int N, const float *w, const float *b, int Cout, int relu,
                     int pool, float sa_in, float sa_out, float *y, float *sw_out) {
    DeviceGuard dg(c);
    if (!c || !x || !w || !b || !y) return LRCN_EINVAL;
    if (W < 2 || H < 2 || (W & 1) || (H & 1) || Cin < 128 || (Cin % 128) || Cout < 128 || (Cout % 16) || N < 1 || (int64_t)N * W * H < 256 ||
        !(sa_in > 0.0f) || !(sa_out > 0.0f))
        FAIL(c, LRCN_EINVAL, "conv3x3_fp8: need even W,H, Cin %% 128 == 0, Cout >= 128 and %% 16 == 0, N*W*H >= 256, positive scales");
    void *xin = nullptr, *wp = nullptr, *out = nullptr;
    float *f = nullptr;  // b, sw, escale, ebias
    const int Wo = pool ? W / 2 : W, Ho = pool ? H / 2 : H;
    auto cleanup = [&]() {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(xin);
        (void)hipFree(wp);
        (void)hipFree(out);
        (void)hipFree(f);
    };
    if (hipMalloc(&xin, (size_t)N * H * W * Cin) != hipSuccess || hipMalloc(&wp, (size_t)Cout * 9 * Cin) != hipSuccess ||
        hipMalloc(&out, (size_t)N * Ho * Wo * Cout) != hipSuccess || hipMalloc((void **)&f, sizeof(float) * 4 * Cout) != hipSuccess) {
        cleanup();
        FAIL(c, LRCN_ENOMEM, "conv3x3_fp8 scratch");
    }
    float *bd = f, *sw = f + Cout, *es = f + 2 * Cout, *eb = f + 3 * Cout;
    (void)hipMemcpyAsync(bd, b, sizeof(float) * Cout, hipMemcpyDeviceToDevice, c->stream);
    k_ref_to_nhwc_fp8(c->stream, x, W, H, Cin, N, 1.0f / sa_in, xin);
    k_quant_conv_w_fp8(c->stream, w, Cin, Cout, wp, sw);
    k_fp8_epilogue_params(c->stream, bd, sw, Cout, sa_in, sa_out, es, eb);
    if (sw_out) (void)hipMemcpyAsync(sw_out, sw, sizeof(float) * Cout, hipMemcpyDeviceToDevice, c->stream);
    GemmArgs g{};
    g.dtype = GEMM_T_F8;
    g.A = xin;
    g.B = wp;
    g.ldb = 9 * Cin;
    g.C = out;
    g.ldc = Cout;
    g.M = N * H * W;
    g.N = Cout;
    g.K = 9 * Cin;
    g.bias = eb;
    g.scale = es;
    g.relu = relu;
    g.a_mode = GEMM_A_CONV3;
    g.out_mode = pool ? GEMM_OUT_POOL : GEMM_OUT_CONV;
    g.H = H;
    g.W = W;
    g.Cin = Cin;
    g.zero_page = c->zero_page;
    hipError_t e = launch_gemm(c->stream, g);
    if (e == hipSuccess) {
        k_nhwc_fp8_to_ref(c->stream, out, Wo, Ho, Cout, N, sa_out, y);
        e = hipGetLastError();
    }
    cleanup();
    if (e != hipSuccess) FAIL(c, LRCN_EHIP, "conv3x3_fp8: %s", hipGetErrorString(e));
    return LRCN_OK;
}

}  // extern "C"
