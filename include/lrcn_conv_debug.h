/* lrcn_conv_debug.h -- conv1_1 of the bf16 stack by itself (conv11.hip), from either of its two source forms: the test entry of the
 * one convolution kernel no other entry reaches alone, beside the C ABI of include/lrcn.h (which it includes; LRCN_ABI_VERSION is
 * unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement this entry point. */
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

#ifdef __cplusplus
}
#endif

#endif /* LRCN_CONV_DEBUG_H */
