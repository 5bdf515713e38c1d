/* lrcn_gemm_debug.h -- one contraction through the GEMM router with caller-given operands: the test entries of the GEMM engines in their
 * plain (lrcn_debug_gemm) and 3x3-convolution (lrcn_debug_conv_gemm) operand modes, beside the C ABI of include/lrcn.h (which it includes;
 * LRCN_ABI_VERSION is unchanged).  Implemented by liblrcn_hip.so only: the CPU oracle does not implement these entry points. */
#ifndef LRCN_GEMM_DEBUG_H
#define LRCN_GEMM_DEBUG_H

#include "lrcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C[M][N] (+)= A[M][K] * B[N][K]^T (+ bias[N]) (ReLU): both operands K-contiguous, row-major with the leading dimensions lda / ldb / ldc in
 * ELEMENTS.  Every pointer is a device pointer that the caller allocated and filled in the element type it names; the entry allocates
 * nothing and converts nothing. */
typedef struct lrcn_gemm_debug {
    int dtype;            /* LRCN_F32 or LRCN_BF16: element type of A and B */
    const void *A;        /* [M][lda] */
    const void *B;        /* [N][ldb] */
    void *C;              /* [M][ldc]: f32 if c_f32 (or dtype is LRCN_F32), else bf16 */
    const float *bias;    /* [N] f32, 16-byte aligned, or NULL */
    int64_t lda, ldb, ldc;
    int M, N, K;          /* K is passed to the engines as given (the library's own callers round it up to the operands' zero padding) */
    int c_f32;            /* bf16 operands: 1 = f32 output */
    int beta;             /* 1: C += result */
    int relu;
    int c_is_zero;        /* the caller guarantees that C holds zeros (a split-K by atomics may then skip its own clearing) */
    int deterministic;    /* 1: no float-atomic split-K */
    int free_cus, bg_cus, wg_cap;   /* the router inputs the library derives from a capped VGG grid (0 = the LSTM runs alone) */
} lrcn_gemm_debug;

/* Fills the router's arguments as the library's own plain contractions do (PLAIN operand and output modes, the context's zero page, its
 * split-K workspace and its stream), launches, and waits for the stream.  Afterwards lrcn_debug_route(ctx, 0) names the rung that ran:
 * "8p:<tile config>", "8p-bg:<tile config>", "skinny", "8p-splitk:<slices>", "glds", "skinny-last", "glds-small", "gemm_nt".
 * LRCN_EINVAL when ctx or g is NULL, dtype is neither LRCN_F32 nor LRCN_BF16, or the router refuses the arguments (it does so on the host,
 * before any launch: C is untouched); LRCN_EHIP for any other HIP error. */
int lrcn_debug_gemm(lrcn_ctx *ctx, const lrcn_gemm_debug *g);

/* One 3x3 convolution (stride 1, zero padding 1) (+ bias[Cout]) (ReLU) (2x2 maximum) through the same router in its CONV3 operand mode: the
 * implicit-GEMM form every VGG layer from conv2_2 on runs in.  As above, every pointer is a device pointer that the caller allocated and
 * filled in the ENGINE's layouts and element type; the entry allocates nothing, converts nothing and never goes to conv64.hip.
 *   y[n][r][q][co] = sum over kh, kw, c of x[n][r + kh - 1][q + kw - 1][c] * w[co][kh * 3 + kw][c]   (terms outside the image are zero) */
typedef struct lrcn_conv_gemm_debug {
    int dtype;            /* LRCN_F32 or LRCN_BF16: element type of x, w and y */
    const void *x;        /* NHWC [N][H][W][Cin] */
    const void *w;        /* [Cout][9][Cin] */
    const float *bias;    /* [Cout] f32, 16-byte aligned, or NULL */
    void *y;              /* [N][H][W] rows of ldc elements; pool: [N][H/2][W/2] rows of ldc elements */
    int64_t ldc;          /* elements, >= Cout */
    int N, H, W, Cin, Cout;
    int relu;
    int pool;             /* 1: the maximum over each 2x2 window (after bias and ReLU) */
    int wg_cap;           /* > 0: at most this many workgroups walk the tiles (what lrcn_vgg_set_wg_cap gives the layers of a forward) */
} lrcn_conv_gemm_debug;

/* Fills the router's arguments as a VGG layer's launch does (CONV3 operand mode, CONV or POOL output mode, K = ldb = 9 Cin, the context's
 * zero page, its split-K workspace and its stream; static tile walk, no tile queues), launches, and waits for the stream.  Afterwards
 * lrcn_debug_route(ctx, 0) names the rung that ran: "8p:<tile config>", "8p-splitk:<slices>", "glds", "glds-small", "gemm_nt".
 * LRCN_EINVAL when ctx or g is NULL, dtype is neither LRCN_F32 nor LRCN_BF16, or the router refuses the arguments (on the host, before any
 * launch: y is untouched); LRCN_EHIP for any other HIP error. */
int lrcn_debug_conv_gemm(lrcn_ctx *ctx, const lrcn_conv_gemm_debug *g);

#ifdef __cplusplus
}
#endif

#endif /* LRCN_GEMM_DEBUG_H */
