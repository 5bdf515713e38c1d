/* lrcn_conv_debug.h -- test entries of the convolution stack's pieces that no other entry reaches alone, beside the C ABI of include/lrcn.h
 * (which it includes; LRCN_ABI_VERSION is unchanged): conv1_1 of the bf16 stack by itself (conv11.hip), from either of its two source
 * forms, conv64.hip's plain halo-patch kernel on the caller's operands under a workgroup cap, and the seams of the fp8 stack (fp8.hip's two casts and its amax, conv2_1's e4m3 epilogue in conv64.hip, the calibrated scales).
 * Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points. */
#ifndef LRCN_CONV_DEBUG_H
#define LRCN_CONV_DEBUG_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* y = relu(conv3x3(x, w11) + b11) in one launch of the kernel lrcn_vgg_forward[_u8] runs for conv1_1 when the fused first launch is off.
 * src: src_is_u8 != 0 -- uint8 crops [N][S][S][3] (x = crop - mean per channel, read_image_data's arithmetic, lrcn.jl:766-772);
 *      src_is_u8 == 0 -- the preprocessed float tensor (S,S,3,N) column-major (mean is ignored and may be NULL).
 * w11 (3,3,3,64) in the reference layout, b11 [64]; y (S,S,64,N) column-major f32 holding the kernel's bf16 values.  Every pointer is a
 * device pointer; scratch is allocated and freed inside the call, as in lrcn_conv1_fused.
 * LRCN_EINVAL before any launch when a pointer is NULL (mean only with a uint8 source), the context's vgg_dtype is LRCN_F32, N < 1, S < 2,
 * S is odd, or N * S * S * 64 does not fit 31 bits; LRCN_ENOMEM / LRCN_EHIP as elsewhere. */
int lrcn_debug_conv11(lrcn_ctx *ctx, const void *src, int src_is_u8, int N, int S, const float mean[3], const float *w11, const float *b11,
                      float *y);

/* One of fp8.hip's two elementwise casts on the caller's device buffers, n elements:
 *   dir == 0: bf16 src[n] -> OCP e4m3 bytes dst[n] = e4m3(clamp(src * factor, +-448))   (k_cast_bf16_fp8: in front of conv2_2 when conv2_1
 *             did not write e4m3 itself; the stack passes factor = 1.0f / scale, formed on the host)
 *   dir != 0: e4m3 bytes src[n] -> bf16 dst[n] = bf16(src * factor)                      (k_cast_fp8_bf16: pool5 -> fc6; factor = scale)
 * `factor` goes to the kernel as given.  LRCN_EINVAL before any launch when a pointer is NULL or not 16-byte aligned, n < 8, n % 8 != 0,
 * factor is not finite or not positive, or the context's vgg_dtype is LRCN_F32.  The stream is drained before the call returns. */
int lrcn_debug_fp8_cast(lrcn_ctx *ctx, int dir, const void *src, int64_t n, float factor, void *dst);

/* *out_dev = max |x[i]| over the n bf16 values at x (device): zeroes *out_dev, then fp8.hip's k_amax, the kernel lrcn_vgg_calibrate collects
 * every layer's output range with (0 for all zeroes; +inf if one is there).  LRCN_EINVAL when a pointer is NULL or n < 1. */
int lrcn_debug_amax(lrcn_ctx *ctx, const void *x_bf16, int64_t n, float *out_dev);

/* conv2_1 as the fp8 stack runs it on conv64.hip, writing conv2_2's e4m3 input itself: y = e4m3(min(relu(conv3x3(x, w) + b) * f8_inv_scale,
 * 448)) from the f32 sum (NOT from its bf16 rounding, which is what the cast route above quantises).  Built like lrcn_conv3x3 on a bf16
 * context with Cin = 64: x (W,H,64,N), w (3,3,64,Cout), b [Cout] in the reference layouts (device float), operands rounded to bf16,
 * the context's workgroup cap (lrcn_vgg_set_wg_cap) applies; y (W,H,Cout,N) f32 holds the e4m3 values undequantised.
 * LRCN_EINVAL before any launch when a pointer is NULL, the context's vgg_dtype is LRCN_F32, W or H is no multiple of 16, Cout no
 * multiple of 64, N < 1, N * W * H * 64 does not fit 31 bits, or f8_inv_scale is not finite or not positive. */
int lrcn_debug_conv64_f8(lrcn_ctx *ctx, const float *x, int W, int H, int N, const float *w, const float *b, int Cout, float f8_inv_scale,
                         float *y);

/* One 3x3 convolution (stride 1, zero padding 1) (+ bias[Cout]) (ReLU) (2x2 maximum) of 64 input channels on conv64.hip's halo-patch kernel
 * (conv64_kernel<pool, false>: conv1_2 and conv2_1 of the bf16 stack), on the caller's operands in the KERNEL's layouts, in the style of
 * lrcn_debug_conv_gemm (include/lrcn_gemm_debug.h): every pointer is a device pointer that the caller allocated and filled; the entry
 * allocates nothing and converts nothing.
 *   y[n][r][q][co] = sum over kh, kw, c of x[n][r + kh - 1][q + kw - 1][c] * w[co][kh * 3 + kw][c]   (terms outside the image are zero) */
typedef struct lrcn_conv64_debug {
    const void *x;        /* bf16, NHWC [N][H][W][64], 16-byte aligned */
    const void *w;        /* bf16, [Cout][9][64], 16-byte aligned */
    const float *bias;    /* [Cout] f32, or NULL: zeros (the launch then carries no bias pointer) */
    void *y;              /* bf16, [N][H][W][Cout]; pool: [N][H/2][W/2][Cout]; 16-byte aligned */
    int N, H, W, Cout;
    int relu;
    int pool;             /* 1: the maximum over each 2x2 window (after bias and ReLU) */
    int wg_cap;           /* what lrcn_vgg_set_wg_cap gives a forward's layers: >= 8 caps the grid at wg_cap / (Cout / 64) workgroups (at
                             least 1) per 64-channel chunk, each walking tiles b, b + G, ...; below 8: 256 / (Cout / 64) */
} lrcn_conv64_debug;

/* launch_conv64 with the context's zero page and stream and the given cap, then waits for the stream.  Afterwards lrcn_debug_route(ctx, 0)
 * is "conv64".  LRCN_EINVAL on the host, before any launch (y is untouched), when ctx, d, x, w or y is NULL, the context's vgg_dtype is
 * LRCN_F32, W or H is no multiple of 16 or below 16, Cout no multiple of 64 or below 64, N < 1, N * H * W * 64 does not fit 31 bits, or x, w
 * or y is not 16-byte aligned; LRCN_EHIP for any HIP error. */
int lrcn_debug_conv64(lrcn_ctx *ctx, const lrcn_conv64_debug *d);

/* Host copy of the per-layer activation scales sa of the most recent lrcn_vgg_calibrate: out[l] for conv layer l = 0 .. 12; entries below
 * conv2_1 (l = 2), whose outputs stay bf16, are 0.  LRCN_ESTATE when the context is not LRCN_FP8 or not yet calibrated. */
int lrcn_debug_fp8_scales(lrcn_ctx *ctx, float out[13]);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_CONV_DEBUG_H */
