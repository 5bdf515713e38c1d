// image_kernels.hip -- the VGG side's kernels (vgg.hip, conv64.hip, conv64f.hip): weight repacks, uint8 image preprocessing, resize +
// crop, conv1_1's im2col, the reference <-> NHWC layout changes, feature normalisation.
#include "kernel_util.h"

namespace {

template <typename T> __global__ void repack_conv_w_kernel(const float *w, int Cin, int Cout, int Cin_pad, T *out) {
    // w(a,b,ci,co) at a + 3*(b + 3*(ci + Cin*co));  out[co][tap=b*3+a][ci]
    const int64_t total = (int64_t)Cout * 9 * Cin_pad;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ci = (int)(i % Cin_pad);
        const int tap = (int)((i / Cin_pad) % 9);
        const int co = (int)(i / ((int64_t)Cin_pad * 9));
        const int b = tap / 3, a = tap - 3 * b;
        out[i] = from_f32<T>(ci < Cin ? w[a + 3 * (b + 3 * ((int64_t)ci + (int64_t)Cin * co))] : 0.0f);
    }
}
template <typename T> __global__ void repack_conv11_w_kernel(const float *w, int Cout, T *out, int64_t ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Cout * ld) return;
    const int k = i % ld, co = i / ld;
    float v = 0.0f;
    if (k < 27) {
        const int tap = k / 3, c = k - 3 * tap;
        const int b = tap / 3, a = tap - 3 * b;
        v = w[a + 3 * (b + 3 * (c + 3 * co))];
    }
    out[i] = from_f32<T>(v);
}
// out[i] = (bf16)(img[i] - mean[i % 3])  : read_image_data's arithmetic (lrcn.jl:770) in the crop's own layout [n][row][col][3]
// avg != NULL: the full averageImage (S,S,3) column-major instead of the three channel means; the reference subtracts it BEFORE
// its last H <-> W permutedims (lrcn.jl:770-771), so pixel (row r, col q, c) meets avg(q, r, c) = avg[q + S r + S^2 c]
__device__ __forceinline__ float avg_at(const float *avg, int64_t i, int S) {
    const int c = (int)(i % 3);
    const int64_t px = i / 3;
    const int q = (int)(px % S), r = (int)((px / S) % S);
    return avg[q + (int64_t)S * r + (int64_t)S * S * c];
}
// PAD = 2: the output is the crop inside a frame of PAD zero pixels on every side, out[n][S + 2 PAD][S + 2 PAD][3] (the frame is zero
// since allocation and never written): conv64.hip's raw-window DMA then reads conv1_1's zero padding as DATA -- no per-lane in-image tests,
// and a dword of the window never straddles the image edge (its element-shifted second copy needs that).
template <int PAD>
__global__ void img_u8_to_bf16_kernel(const uint8_t *img, int64_t n, float m0, float m1, float m2, const float *avg, int S, bf16_t *out) {
    // 12 bytes (4 pixels) per thread: channel phase is the same for every thread; S % 4 == 0, so the four pixels share an image row
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i0 = t * 12;
    if (i0 >= n) return;
    const int SP = S + 2 * PAD;
    auto opix = [&](int64_t pix) {  // flat pixel index (n, x, y) -> pixel index in the framed output
        const int64_t row = pix / S;           // n * S + x
        const int y = (int)(pix - row * S);
        const int64_t nn = row / S;
        const int x = (int)(row - nn * S);
        return ((nn * SP + x + PAD) * SP + y + PAD);
    };
    if (avg) {
        for (int64_t i = i0; i < n && i < i0 + 12; ++i) out[opix(i / 3) * 3 + i % 3] = (bf16_t)((float)img[i] - avg_at(avg, i, S));
        return;
    }
    if (i0 + 12 <= n && (S & 3) == 0) {
        const uint32_t *p = reinterpret_cast<const uint32_t *>(img + i0);
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
        const float mean[3] = {m0, m1, m2};
        bf16_t o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const uint32_t w = k < 4 ? w0 : (k < 8 ? w1 : w2);
            o[k] = (bf16_t)((float)((w >> (8 * (k & 3))) & 0xFFu) - mean[k % 3]);
        }
        // 24 bytes at a 4-byte-aligned address (the framed pixel index of a thread's first pixel is even)
        uint32_t *q = reinterpret_cast<uint32_t *>(out + opix(i0 / 3) * 3);
        const uint32_t *ov = reinterpret_cast<const uint32_t *>(o);
#pragma unroll
        for (int k = 0; k < 6; ++k) q[k] = ov[k];
    } else {
        for (int64_t i = i0; i < n && i < i0 + 12; ++i)
            out[opix(i / 3) * 3 + i % 3] = (bf16_t)((float)img[i] - (i % 3 == 0 ? m0 : (i % 3 == 1 ? m1 : m2)));
    }
}
// conv1_1 weights for the fused conv1_1+conv1_2 kernels (conv64.hip FUSE, conv64f.hip): out[co][k'], k' = 8 lq + j:
//   lq < 3: kw = lq, kh = j / 3, c = j % 3 (the first 8 bytes of the 9-byte run of image row kw);  lq = 3: j < 3 -> kw = j, kh = 2, c = 2;
//   k' = 27, 28, 29: the f32 bias of channel co cut into three bf16 pieces, hi + mid + lo = b exactly (24 bits of mantissa in 3 x 8) --
//   conv64f.hip's im2col fragment holds 1.0 there, so the bias enters the f32 accumulation as data; conv64.hip's fragment holds 0 there.
__global__ void repack_conv11_w_fused_kernel(const float *w, const float *b, bf16_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 64 * 32) return;
    const int k = i & 31, co = i >> 5, lq = k >> 3, j = k & 7;
    float v = 0.0f;
    int kw = -1, kh = 0, c = 0;
    if (lq < 3) {
        kw = lq; kh = j / 3; c = j % 3;
    } else if (j < 3) {
        kw = j; kh = 2; c = 2;
    }
    if (kw >= 0) v = w[kw + 3 * (kh + 3 * (c + 3 * co))];  // reference layout (3,3,3,64) column-major: a = kw (dim 1), b = kh (dim 2)
    if (lq == 3 && j >= 3 && j < 6 && b) {
        float rest = b[co];
        for (int piece = 3; piece <= j; ++piece) {
            v = (float)(bf16_t)rest;
            rest -= v;
        }
    }
    out[i] = (bf16_t)v;
}
template <typename T> __global__ void repack_fc6_w_kernel(const float *w, T *out) {
    // out[o][(y*7+x)*512 + c] = w(o, x + 7y + 49c) = w[o + 4096*(x + 7y + 49c)]; tiled through LDS for coalescing both ways
    __shared__ float tile[32][33];
    const int k0 = blockIdx.x * 32, o0 = blockIdx.y * 32;  // k = internal index
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i;  // internal k -> ref k
        const int c = k % 512, yx = k / 512, y = yx / 7, x = yx - 7 * y;
        const int kref = x + 7 * y + 49 * c;
        tile[i][tx] = w[(int64_t)(o0 + tx) + 4096ll * kref];
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) out[(int64_t)(o0 + i) * 25088 + k0 + tx] = from_f32<T>(tile[tx][i]);
}

template <typename T, bool U8>
__global__ void im2col11_kernel(const void *src, int N, int S, float m0, float m1, float m2, T *out, int64_t ld) {
    // one thread per (m, tap); writes 3 channels.  internal (y, x) = (dim 2, dim 1) of the reference tensor;
    // for the uint8 path reference dim 1 = image row, dim 2 = image col (lrcn.jl:766-771).
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t M = (int64_t)N * S * S;
    if (idx >= M * 9) return;  // columns [27, ld) are never read: the GEMM loader masks k >= K = 27
    const int tap = (int)(idx % 9);
    const int m = (int)(idx / 9);
    T *row = out + (int64_t)m * ld;
    const PixDecode p = decode_pixel(m, S, S);
    const int kh = tap / 3, kw = tap - 3 * kh;
    const int y = p.y + kh - 1, x = p.x + kw - 1;
    float v[3] = {0.0f, 0.0f, 0.0f};
    if ((unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S) {
        if (U8) {
            const uint8_t *px = reinterpret_cast<const uint8_t *>(src) + (((int64_t)p.n * S + x) * S + y) * 3;  // row=x, col=y
            v[0] = (float)px[0] - m0;
            v[1] = (float)px[1] - m1;
            v[2] = (float)px[2] - m2;
        } else {
            const float *f = reinterpret_cast<const float *>(src);
            for (int c = 0; c < 3; ++c) v[c] = f[(int64_t)x + (int64_t)S * (y + (int64_t)S * (c + 3ll * p.n))];
        }
    }
    for (int c = 0; c < 3; ++c) row[tap * 3 + c] = from_f32<T>(v[c]);
}

__global__ void preprocess_u8_kernel(const uint8_t *img, int N, int S, float m0, float m1, float m2, const float *avg, float *out) {
    const int64_t total = (int64_t)N * 3 * S * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int ii = (int)(i % S), j = (int)((i / S) % S), c = (int)((i / ((int64_t)S * S)) % 3);
        const int n = (int)(i / (3ll * S * S));
        const float mean = avg ? avg[j + (int64_t)S * ii + (int64_t)S * S * c] : (c == 0 ? m0 : (c == 1 ? m1 : m2));
        out[i] = (float)img[(((int64_t)n * S + ii) * S + j) * 3 + c] - mean;
    }
}

// read_image_data's geometry (lrcn.jl:755-765) for a batch of decoded images of different sizes: resize so that the shorter side is
// 224 and the other div(side * 224, shorter) (:756), centre crop at div offsets (:758-760), grey -> three channels (:762-764).
// Resampling: bilinear between pixel CENTRES (output (R, Q) of the nh x nw resized image samples the source at
// ((2R+1) h / (2 nh) - 1/2, (2Q+1) w / (2 nw) - 1/2), clamped to the image), computed in exact integer arithmetic with
// round-half-up, so that a host restatement reproduces every byte (Images.imresize's own kernel is unpinned).
struct ImgMeta {
    int64_t off;
    int h, w, ch, pad;
};
__global__ void resize_crop_u8_kernel(const uint8_t *src, const ImgMeta *meta, int N, int S, uint8_t *out) {
    const int64_t total = (int64_t)N * S * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(i % S), r = (int)((i / S) % S), n = (int)(i / ((int64_t)S * S));
        const ImgMeta m = meta[n];
        const int64_t h = m.h, w = m.w, sm = h < w ? h : w;
        const int64_t nh = h * S / sm, nw = w * S / sm;          // :756  div(size * 224, minimum(size))
        const int64_t R = r + (nh - S) / 2, Q = q + (nw - S) / 2;  // :758-760
        int64_t ny = (2 * R + 1) * h - nh, nx = (2 * Q + 1) * w - nw;  // 2 nh * sy, 2 nw * sx
        if (ny < 0) ny = 0;
        if (nx < 0) nx = 0;
        const int64_t y0 = ny / (2 * nh), fy = ny - y0 * 2 * nh, x0 = nx / (2 * nw), fx = nx - x0 * 2 * nw;
        const int64_t y1 = y0 + 1 < h ? y0 + 1 : h - 1, x1 = x0 + 1 < w ? x0 + 1 : w - 1;
        const uint8_t *im = src + m.off;
        const int ch = m.ch;
        uint8_t v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cs = ch >= 3 ? c : 0;
            const int64_t p00 = im[(y0 * w + x0) * ch + cs], p01 = im[(y0 * w + x1) * ch + cs], p10 = im[(y1 * w + x0) * ch + cs],
                          p11 = im[(y1 * w + x1) * ch + cs];
            const int64_t top = (2 * nw - fx) * p00 + fx * p01, bot = (2 * nw - fx) * p10 + fx * p11;
            v[c] = (uint8_t)(((2 * nh - fy) * top + fy * bot + 2 * nh * nw) / (4 * nh * nw));
        }
        uint8_t *o = out + i * 3;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    }
}

// feats(n, :) /= sum(feats(n, :))  (generate's input/sum(input), lrcn.jl:595-597; what the reference's `featsn` files hold).
// feats: N x F column-major f32; one workgroup per row.
__global__ void normalize_rows_kernel(float *feats, int N, int F) {
    __shared__ float sh[8];
    const int n = blockIdx.x;
    float s = 0.0f;
    for (int j = threadIdx.x; j < F; j += blockDim.x) s += feats[n + (int64_t)N * j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    float tot = 0.0f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += sh[w];
    for (int j = threadIdx.x; j < F; j += blockDim.x) feats[n + (int64_t)N * j] /= tot;
}

template <typename T> __global__ void ref_to_nhwc_kernel(const float *x, int W, int H, int C, int N, T *out, int C_ld) {
    const int64_t total = (int64_t)N * H * W * C_ld;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C_ld);
        const int xx = (int)((i / C_ld) % W), yy = (int)((i / ((int64_t)C_ld * W)) % H);
        const int n = (int)(i / ((int64_t)C_ld * W * H));
        out[i] = from_f32<T>(c < C ? x[(int64_t)xx + (int64_t)W * (yy + (int64_t)H * (c + (int64_t)C * n))] : 0.0f);
    }
}
template <typename T> __global__ void nhwc_to_ref_kernel(const T *in, int W, int H, int C, int N, int C_ld, float *out) {
    const int64_t total = (int64_t)N * C * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % W), yy = (int)((i / W) % H), c = (int)((i / ((int64_t)W * H)) % C);
        const int n = (int)(i / ((int64_t)W * H * C));
        out[i] = to_f32(in[(((int64_t)n * H + yy) * W + xx) * C_ld + c]);
    }
}

}  // namespace
// ---------------------------------------------------------------- launchers
void k_repack_conv_w(hipStream_t st, int dtype, const float *w, int Cin, int Cout, int Cin_pad, void *out) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(repack_conv_w_kernel<T>, dim3(grid1d((int64_t)Cout * 9 * Cin_pad)), dim3(256), 0, st,
                                         w, Cin, Cout, Cin_pad, (T *)out));
}
void k_repack_conv11_w(hipStream_t st, int dtype, const float *w, int Cout, void *out, int64_t ld) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(repack_conv11_w_kernel<T>, dim3(cdiv(Cout * ld, 256)), dim3(256), 0, st, w, Cout,
                                         (T *)out, ld));
}
void k_img_u8_to_bf16(hipStream_t st, const uint8_t *img, int64_t n, float m0, float m1, float m2, const float *avg, int S, void *out) {
    const int64_t threads = (n + 11) / 12;
    hipLaunchKernelGGL(img_u8_to_bf16_kernel<2>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, img, n, m0, m1, m2, avg, S,
                       (bf16_t *)out);
}
void k_resize_crop_u8(hipStream_t st, const uint8_t *src, const void *meta, int N, int S, uint8_t *out) {
    hipLaunchKernelGGL(resize_crop_u8_kernel, dim3(grid1d((int64_t)N * S * S)), dim3(256), 0, st, src, (const ImgMeta *)meta, N, S, out);
}
void k_normalize_rows(hipStream_t st, float *feats, int N, int F) {
    hipLaunchKernelGGL(normalize_rows_kernel, dim3(N), dim3(256), 0, st, feats, N, F);
}
void k_repack_conv11_w_fused(hipStream_t st, const float *w, const float *b, void *out) {
    hipLaunchKernelGGL(repack_conv11_w_fused_kernel, dim3(8), dim3(256), 0, st, w, b, (bf16_t *)out);
}
void k_repack_fc6_w(hipStream_t st, int dtype, const float *w, void *out) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(repack_fc6_w_kernel<T>, dim3(25088 / 32, 4096 / 32), dim3(256), 0, st, w, (T *)out));
}
void k_im2col11_u8(hipStream_t st, int dtype, const uint8_t *img, int N, int S, float m0, float m1, float m2, void *out,
                   int64_t ld) {
    const int64_t n = (int64_t)N * S * S * 9;
    DISPATCH_T(dtype, hipLaunchKernelGGL((im2col11_kernel<T, true>), dim3(cdiv(n, 256)), dim3(256), 0, st, (const void *)img,
                                         N, S, m0, m1, m2, (T *)out, ld));
}
void k_im2col11_f32(hipStream_t st, int dtype, const float *x, int N, int S, void *out, int64_t ld) {
    const int64_t n = (int64_t)N * S * S * 9;
    DISPATCH_T(dtype, hipLaunchKernelGGL((im2col11_kernel<T, false>), dim3(cdiv(n, 256)), dim3(256), 0, st, (const void *)x, N,
                                         S, 0.f, 0.f, 0.f, (T *)out, ld));
}
void k_preprocess_u8(hipStream_t st, const uint8_t *img, int N, int S, float m0, float m1, float m2, const float *avg, float *out) {
    hipLaunchKernelGGL(preprocess_u8_kernel, dim3(grid1d((int64_t)N * 3 * S * S)), dim3(256), 0, st, img, N, S, m0, m1, m2, avg,
                       out);
}
void k_ref_to_nhwc(hipStream_t st, int dtype, const float *x, int W, int H, int C, int N, void *out, int C_ld) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(ref_to_nhwc_kernel<T>, dim3(grid1d((int64_t)N * H * W * C_ld)), dim3(256), 0, st, x,
                                         W, H, C, N, (T *)out, C_ld));
}
void k_nhwc_to_ref(hipStream_t st, int dtype, const void *in, int W, int H, int C, int N, int C_ld, float *out) {
    DISPATCH_T(dtype, hipLaunchKernelGGL(nhwc_to_ref_kernel<T>, dim3(grid1d((int64_t)N * C * H * W)), dim3(256), 0, st,
                                         (const T *)in, W, H, C, N, C_ld, out));
}
