// cider.hip -- CIDEr-D over token ids on the device (include/lrcn_cider.h): the reward of self-critical training without the host loop.
// The tables are built on the host by cider_table.h (plain C++) and uploaded once; the one kernel is
//   cider_score_kernel -- one workgroup of one wave64 per hypothesis.  The row's words are staged in LDS.  Per n = 1..4:
//                           1. lane l owns the n-gram positions l, l + 64, l + 128, l + 192; an all-pairs compare in LDS (every lane reads the
//                              same position j at a time: broadcast reads) tells it whether its position is the n-gram's first and how often
//                              the n-gram occurs
//                           2. each first occurrence probes the n-gram hash table (full-key compare): slot and idf, one dependent load level
//                              per probe step
//                           3. |v_h|^2: the lane's own squares in position order, then an xor tree over the lanes
//                           4. per reference of the image, in order: the reference's (slot, count) pairs are read at wave-uniform addresses
//                              (no search, no address that depends on loaded data) and compared with the lane's slots; the clipped products go
//                              through the same lane-serial-then-tree sum; lane 0 applies the penalty and the norms
//                         All floating point is double and no sum uses an atomic, so a score depends on the caption, the image and the tables
//                         alone.
#include <cmath>
#include <cstring>

#include "../../include/lrcn_cider.h"
#include "cider_table.h"
#include "host.h"

using namespace lrcn_impl;
namespace ch = lrcn_cider_host;

namespace {

constexpr int CIDER_MAXW = LRCN_CIDER_MAXWORDS;   // 256
constexpr int CIDER_PER_LANE = CIDER_MAXW / 64;   // n-gram positions per lane

struct CiderDev {
    const int32_t *keys[4];
    const double *idf[4];
    uint32_t mask[4];
    const ch::Entry *ent[4];
    const int32_t *ent_off[4];
    const double *rnorm[4];
    const int32_t *ref_len, *img_off, *img_ref;
    double log_n;
    int n_images;
};

// the sum of v over the 64 lanes in a fixed tree; every lane gets it
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int N>
__device__ __forceinline__ bool same_ngram(const int32_t *a, const int32_t *b) {
    bool eq = true;
#pragma unroll
    for (int k = 0; k < N; ++k) eq = eq && a[k] == b[k];
    return eq;
}

// One order n of one hypothesis (nw words in LDS `w`, which has N - 1 readable ints of padding behind them): adds this order's terms to
// acc[], one slot per reference of the image (lane 0's copy is the one that counts).
template <int N>
__device__ __forceinline__ void cider_order(const CiderDev &t, const int32_t *w, int nw, int r0, int nref, double *acc_lds) {
    const int lane = threadIdx.x;
    const int P = nw - N + 1;   // n-gram positions
    if (P <= 0) return;         // |v_h| = 0: every term of this order is skipped
    int32_t slot[CIDER_PER_LANE];
    double vh[CIDER_PER_LANE];
    double sq = 0.0;
#pragma unroll
    for (int q = 0; q < CIDER_PER_LANE; ++q) {
        const int p = lane + 64 * q;
        slot[q] = -2;   // no first occurrence here: matches no entry
        vh[q] = 0.0;
        if (p < P) {
            bool first = true;
            int cnt = 0;
            for (int j = 0; j < P; ++j) {
                const bool eq = same_ngram<N>(w + p, w + j);
                first = first && !(eq && j < p);
                cnt += eq ? 1 : 0;
            }
            if (first) {
                bool in_range = true;   // a negative id (the device form's contract) must not meet the empty-slot mark
#pragma unroll
                for (int k = 0; k < N; ++k) in_range = in_range && w[p + k] >= 0;
                int32_t found = -1;
                if (in_range) {
                    uint32_t s = ch::cider_hash(w + p, N) & t.mask[N - 1];
                    for (uint32_t step = 0; step <= t.mask[N - 1]; ++step) {   // (the table is at most half full: an empty slot ends it)
                        const int32_t *k = t.keys[N - 1] + (size_t)s * N;
                        if (k[0] < 0) break;
                        if (same_ngram<N>(k, w + p)) {
                            found = (int32_t)s;
                            break;
                        }
                        s = (s + 1) & t.mask[N - 1];
                    }
                }
                slot[q] = found;   // -1: in no reference, idf = log N, meets no entry either
                vh[q] = (double)cnt * (found >= 0 ? t.idf[N - 1][found] : t.log_n);
                sq += vh[q] * vh[q];
            }
        }
    }
    const double hn = sqrt(wave_sum(sq));
    if (hn == 0.0) return;   // wave-uniform
    for (int k = 0; k < nref; ++k) {
        const int r = t.img_ref[r0 + k];
        const double rn = t.rnorm[N - 1][r];
        if (rn == 0.0) continue;   // wave-uniform
        const int e0 = t.ent_off[N - 1][r], e1 = t.ent_off[N - 1][r + 1];
        int32_t cr[CIDER_PER_LANE];
#pragma unroll
        for (int q = 0; q < CIDER_PER_LANE; ++q) cr[q] = 0;
        for (int e = e0; e < e1; ++e) {
            const ch::Entry en = t.ent[N - 1][e];   // the same address in every lane
#pragma unroll
            for (int q = 0; q < CIDER_PER_LANE; ++q) cr[q] = slot[q] == en.slot ? en.count : cr[q];
        }
        double dot = 0.0;
#pragma unroll
        for (int q = 0; q < CIDER_PER_LANE; ++q) {
            if (cr[q] > 0) {
                const double vr = (double)cr[q] * t.idf[N - 1][slot[q]];
                dot += fmin(vh[q], vr) * vr;
            }
        }
        dot = wave_sum(dot);
        if (lane == 0) {
            const double d = (double)(nw - t.ref_len[r]);
            const double pen = exp(-(d * d) / 72.0);
            acc_lds[k & 63] += pen * dot / (hn * rn);
        }
    }
}

__global__ __launch_bounds__(64) void cider_score_kernel(CiderDev t, const int32_t *tokens, int ld, const int32_t *out_len,
                                                         const int32_t *image, int R, double *out) {
    __shared__ int32_t w[CIDER_MAXW + 4];
    __shared__ double acc[64];   // lane 0's per-reference sums; reference k uses slot k mod 64 (the sum over k stays in k order per slot)
    const int row = blockIdx.x, lane = threadIdx.x;
    if (row >= R) return;
    const int len = out_len[row], img = image[row];
    if (len < 2 || len > ld || img < 0 || img >= t.n_images) {
        if (lane == 0) out[row] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const int32_t *src = tokens + (size_t)row * ld;
    const int nw = len - 1 - (src[len - 1] == LRCN_EOS ? 1 : 0);
    if (nw > CIDER_MAXW) {
        if (lane == 0) out[row] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const int r0 = t.img_off[img], nref = t.img_off[img + 1] - r0;
    if (nw == 0 || nref == 0) {
        if (lane == 0) out[row] = 0.0;
        return;
    }
    for (int i = lane; i < CIDER_MAXW + 4; i += 64) w[i] = i < nw ? src[1 + i] : -1;
    acc[lane] = 0.0;
    __syncthreads();
    cider_order<1>(t, w, nw, r0, nref, acc);
    cider_order<2>(t, w, nw, r0, nref, acc);
    cider_order<3>(t, w, nw, r0, nref, acc);
    cider_order<4>(t, w, nw, r0, nref, acc);
    if (lane == 0) {
        double total = 0.0;
        const int used = nref < 64 ? nref : 64;
        for (int k = 0; k < used; ++k) total += acc[k];
        out[row] = 10.0 * total / (4.0 * (double)nref);
    }
}

}  // namespace

struct lrcn_cider {
    struct {
        int device;
    } cfg{};
    std::string err;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    CiderDev dev{};
    lrcn_cider_stats_t stats{};
    int V = 0;
    // staging of lrcn_cider_score, grown to the largest call: pinned [tokens R*ld | out_len R | image R] and its device copy, out R doubles
    int32_t *h_in = nullptr, *d_in = nullptr;
    double *h_out = nullptr, *d_out = nullptr;
    size_t in_cap = 0, out_cap = 0;
};

namespace {

std::string g_cider_create_err;

template <class T> int cider_upload(lrcn_cider *c, const T *&dst, const std::vector<T> &src) {
    T *p = nullptr;
    DALLOC(c, p, sizeof(T) * src.size());
    if (!src.empty()) HIPCHK(c, hipMemcpy(p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    c->stats.device_bytes += (int64_t)(sizeof(T) * src.size());
    dst = p;
    return LRCN_OK;
}
#define CUP(...)                            \
    do {                                    \
        int _r = cider_upload(__VA_ARGS__); \
        if (_r) return _r;                  \
    } while (0)

int cider_create_impl(lrcn_cider *c, const ch::Tables &t) {
    CiderDev &d = c->dev;
    d.log_n = t.log_n;
    d.n_images = t.n_images;
    c->stats.images = t.n_images;
    c->stats.references = t.n_refs;
    for (int q = 0; q < 4; ++q) {
        d.mask[q] = t.slots[q] - 1;
        c->stats.ngrams[q] = t.ngrams[q];
        c->stats.slots[q] = t.slots[q];
        c->stats.ref_entries[q] = (int64_t)t.ent[q].size();
        CUP(c, d.keys[q], t.keys[q]);
        CUP(c, d.idf[q], t.idf[q]);
        CUP(c, d.ent[q], t.ent[q]);
        CUP(c, d.ent_off[q], t.ent_off[q]);
        CUP(c, d.rnorm[q], t.rnorm[q]);
    }
    CUP(c, d.ref_len, t.ref_len);
    CUP(c, d.img_off, t.img_off);
    CUP(c, d.img_ref, t.img_ref);
    return LRCN_OK;
}

int cider_launch(lrcn_cider *c, const int32_t *tokens, int ld, const int32_t *out_len, const int32_t *image, int R, double *out) {
    hipLaunchKernelGGL(cider_score_kernel, dim3((unsigned)R), dim3(64), 0, c->stream, c->dev, tokens, ld, out_len, image, R, out);
    KCHK(c, "cider_score_kernel");
    return LRCN_OK;
}

int cider_reserve(lrcn_cider *c, size_t in_ints, size_t out_doubles) {
    if (in_ints > c->in_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->h_in) (void)hipHostFree(c->h_in);
        if (c->d_in) (void)hipFree(c->d_in);
        c->h_in = c->d_in = nullptr;
        c->in_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->h_in, sizeof(int32_t) * in_ints, hipHostMallocDefault));
        HIPCHK(c, hipMalloc((void **)&c->d_in, sizeof(int32_t) * in_ints));
        c->in_cap = in_ints;
    }
    if (out_doubles > c->out_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->h_out) (void)hipHostFree(c->h_out);
        if (c->d_out) (void)hipFree(c->d_out);
        c->h_out = c->d_out = nullptr;
        c->out_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->h_out, sizeof(double) * out_doubles, hipHostMallocDefault));
        HIPCHK(c, hipMalloc((void **)&c->d_out, sizeof(double) * out_doubles));
        c->out_cap = out_doubles;
    }
    return LRCN_OK;
}

}  // namespace

extern "C" {

const char *lrcn_cider_last_error(const lrcn_cider *c) { return c ? c->err.c_str() : g_cider_create_err.c_str(); }

void lrcn_cider_destroy(lrcn_cider *c) {
    if (!c) return;
    DeviceGuard dg(c->cfg.device);
    (void)hipDeviceSynchronize();
    for (void *p : c->allocs) (void)hipFree(p);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->d_in) (void)hipFree(c->d_in);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->d_out) (void)hipFree(c->d_out);
    delete c;
}

int lrcn_cider_create(int device, int n_images, int n_refs, const int32_t *ref_image, const int64_t *ref_offsets, const int32_t *ref_tokens, int V,
                      lrcn_cider **out) {
    if (!out) {
        g_cider_create_err = "null output pointer";
        return LRCN_EINVAL;
    }
    *out = nullptr;
    ch::Tables t;
    const std::string msg = ch::build_tables(n_images, n_refs, ref_image, ref_offsets, ref_tokens, V, t);
    if (!msg.empty()) {
        g_cider_create_err = msg;
        return LRCN_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_cider_create_err = "device " + std::to_string(device) + " not present";
        return LRCN_EINVAL;
    }
    DeviceGuard dg(device);
    lrcn_cider *c = new lrcn_cider();
    c->cfg.device = device;
    c->V = V;
    const int r = cider_create_impl(c, t);
    if (r) {
        g_cider_create_err = c->err;
        lrcn_cider_destroy(c);
        return r;
    }
    *out = c;
    return LRCN_OK;
}

int lrcn_cider_set_stream(lrcn_cider *c, void *stream) {
    if (!c) return LRCN_EINVAL;
    c->stream = reinterpret_cast<hipStream_t>(stream);
    return LRCN_OK;
}

int lrcn_cider_stats(const lrcn_cider *c, lrcn_cider_stats_t *out) {
    if (!c || !out) return LRCN_EINVAL;
    *out = c->stats;
    return LRCN_OK;
}

int lrcn_cider_score_dev(lrcn_cider *c, const int32_t *tokens, int ld, const int32_t *out_len, const int32_t *image, int R, double *out) {
    if (!c) return LRCN_EINVAL;
    if (!tokens || !out_len || !image || !out) FAIL(c, LRCN_EINVAL, "null pointer");
    if (R < 1) FAIL(c, LRCN_EINVAL, "R=%d must be >= 1", R);
    if (ld < 2) FAIL(c, LRCN_EINVAL, "ld=%d must be >= 2", ld);
    DeviceGuard dg(c->cfg.device);
    return cider_launch(c, tokens, ld, out_len, image, R, out);
}

int lrcn_cider_score(lrcn_cider *c, const int32_t *tokens, int ld, const int32_t *out_len, const int32_t *image, int R, double *out) {
    if (!c) return LRCN_EINVAL;
    if (!tokens || !out_len || !image || !out) FAIL(c, LRCN_EINVAL, "null pointer");
    if (R < 1) FAIL(c, LRCN_EINVAL, "R=%d must be >= 1", R);
    if (ld < 2) FAIL(c, LRCN_EINVAL, "ld=%d must be >= 2", ld);
    for (int r = 0; r < R; ++r) {
        if (image[r] < 0 || image[r] >= c->dev.n_images) FAIL(c, LRCN_EINVAL, "row %d: image %d outside [0,%d)", r, image[r], c->dev.n_images);
        if (out_len[r] < 2 || out_len[r] > ld) FAIL(c, LRCN_EINVAL, "row %d: out_len %d outside [2,%d]", r, out_len[r], ld);
        const int32_t *row = tokens + (size_t)r * ld;
        const int nw = out_len[r] - 1 - (row[out_len[r] - 1] == LRCN_EOS ? 1 : 0);
        if (nw > CIDER_MAXW) FAIL(c, LRCN_EINVAL, "row %d: %d words, more than %d", r, nw, CIDER_MAXW);
        for (int k = 1; k <= nw; ++k)
            if (row[k] < 0 || row[k] >= c->V) FAIL(c, LRCN_EINVAL, "row %d: word %d is %d, outside [0,%d)", r, k - 1, row[k], c->V);
    }
    DeviceGuard dg(c->cfg.device);
    const size_t n_tok = (size_t)R * ld, n_in = n_tok + 2 * (size_t)R;
    int rc = cider_reserve(c, n_in, (size_t)R);
    if (rc) return rc;
    memcpy(c->h_in, tokens, sizeof(int32_t) * n_tok);
    memcpy(c->h_in + n_tok, out_len, sizeof(int32_t) * R);
    memcpy(c->h_in + n_tok + R, image, sizeof(int32_t) * R);
    HIPCHK(c, hipMemcpyAsync(c->d_in, c->h_in, sizeof(int32_t) * n_in, hipMemcpyHostToDevice, c->stream));
    rc = cider_launch(c, c->d_in, ld, c->d_in + n_tok, c->d_in + n_tok + R, R, c->d_out);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, sizeof(double) * R, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, c->h_out, sizeof(double) * R);
    return LRCN_OK;
}

}  // extern "C"
