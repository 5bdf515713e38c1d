// host.h -- host plumbing of the caption model (lrcn_api.hip, train*.hip, update.hip, decode.hip, vgg.hip) and activity recognition (activity.hip).  Nothing here
// knows a context: the macros, the device guard and the allocator work on any handle with `std::string err` (the allocator: and `allocs`).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/lrcn.h"
#include "common.h"
#include "gemm.h"
#include "kernels.h"
#include "knob.h"

#define FAIL(ctx, code, ...)                          \
    do {                                              \
        char _b[512];                                 \
        snprintf(_b, sizeof(_b), __VA_ARGS__);        \
        (ctx)->err = _b;                              \
        return (code);                                \
    } while (0)
#define HIPCHK(ctx, expr)                                                                        \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) FAIL(ctx, LRCN_EHIP, "%s: %s", #expr, hipGetErrorString(_e));      \
    } while (0)
#define KCHK(ctx, what)                                                                          \
    do {                                                                                         \
        hipError_t _e = hipGetLastError();                                                       \
        if (_e != hipSuccess) FAIL(ctx, LRCN_EHIP, "%s: %s", what, hipGetErrorString(_e));       \
    } while (0)

namespace lrcn_impl {

// Every entry point that takes a handle runs on the handle's device, whatever device the calling thread had selected,
// and restores the caller's selection on return (allocations, null-stream work and hipFuncSetAttribute are per device).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {  // device < 0: no switch
        if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    template <class Handle> explicit DeviceGuard(const Handle *h) : DeviceGuard(h ? h->cfg.device : -1) {}  // NULL: no switch
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// A zero-filled device buffer, freed with the handle (h->allocs).
template <class Handle, class P> int dalloc(Handle *h, P *&p, size_t bytes) {
    void *q = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) FAIL(h, LRCN_ENOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
    h->allocs.push_back(q);
    p = reinterpret_cast<P *>(q);
    // K-padding columns must hold zeros (never NaN) from the start.  The fill runs on the NULL stream and a device-memory hipMemset may
    // return before it has executed; work that the caller then queues on a NON-BLOCKING stream (torch's side streams, the context's
    // weight-gradient / group streams) is not ordered behind the null stream -- a buffer allocated lazily inside a step could be
    // zeroed AFTER its first kernel had written it (found with tools/fake_multi_check.py: the second shadow set, allocated by the
    // first fused update, lost what the group streams' Adam kernels had just written).  Drain the null stream before handing it out.
    if (hipMemset(q, 0, bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) FAIL(h, LRCN_EHIP, "hipMemset failed");
    return LRCN_OK;
}
#define DALLOC(h, p, bytes)                                    \
    do {                                                       \
        int _r = lrcn_impl::dalloc(h, p, (size_t)(bytes));     \
        if (_r) return _r;                                     \
    } while (0)

// leading dimensions: whole 64-element K-steps, so the direct-to-LDS GEMM can run with K rounded up (pads are zero)
inline int64_t ld64(int64_t n) { return round_up64(n, 64); }
inline char *boff(void *p, int64_t elems, size_t esz) { return reinterpret_cast<char *>(p) + elems * (int64_t)esz; }
inline const char *boff(const void *p, int64_t elems, size_t esz) {
    return reinterpret_cast<const char *>(p) + elems * (int64_t)esz;
}

// The K a GEMM runs with.  bf16: K rounded up to whole 128-byte K-steps.  Every internal operand has ld >= that and zero (weights:
// written zeros; activations: zero or stale-but-finite values that meet a zero on the other side) in the padding.
inline int gemm_k(int dtype, int64_t lda, int64_t ldb, int K) {
    return (dtype == GEMM_T_BF16 && lda >= round_up64(K, 64) && ldb >= round_up64(K, 64)) ? (int)round_up64(K, 64) : K;
}

// The fused bf16 step kernels of lstm_fused.hip (GEMM + cell in one launch per step) for a recurrence of B rows, up to kLstmFusedMaxRows:
// from 256 rows their LDS-heavy workgroups take more from convolutions running beside them than the separate launches do (lstm_fused.hip).
// LRCN_LSTM_FUSED=0: GEMM + cell as separate launches at every batch size.
constexpr int kLstmFusedMaxRows = 128;
inline bool lstm_fused_on(int dtype, int B, int H, int64_t ldH, int64_t ld4H) {
    return !knob_off("LRCN_LSTM_FUSED") && B <= kLstmFusedMaxRows && lstm_fused_eligible(dtype, B, H, ldH, ld4H);
}

// One LSTM layer's recurrence over S steps of B rows (row m = s*B + b) on a handle `h` (lrcn_ctx, lrcn_act: stream, dt, esz, zero_page,
// [B][H] f32 scratch dc / dhrec, err), in the fused form (lstm_fused_on; `alone`: nothing runs beside it) or the plain one, per step the
// recurrent GEMM `gemm(A, lda, B, ldb, C, ldc, M, N, K, beta, c_is_zero)` (C f32 (+)= A B', no bias) and the cell kernel.  Gx f32 [S*B][4H]
// holds the input-side pre-activations (+bias) on entry and the full pre-activations on exit; acts (T) [S*B][ld4H], Call f32 [S*B][H] and
// Hall (T) [S*B][ldH] receive the per-step results (lrcn.jl:528-538, time-batched).  The caller checks the launches (KCHK).
// Step s of that recurrence alone (`fused`: lstm_fused_on of the layer): rows [s*B, (s+1)*B) of Gx hold the step's input-side pre-activations,
// steps < s are complete.  lstm_recurrence_fwd's loop body, and what the stepwise forward of scheduled sampling (train.hip) calls per step.
template <class Handle, class Gemm>
int lstm_step_fwd(Handle *h, bool alone, const Gemm &gemm, bool fused, int s, int B, int H, int64_t ldH, int64_t ld4H, float *Gx,
                  const void *Wh, void *acts, float *Call, void *Hall) {
    float *G = Gx + (int64_t)s * B * 4 * H;
    if (s > 0 && fused) {  // recurrent GEMM + cell in one launch (small batches: launch-latency bound otherwise)
        hipError_t e = launch_lstm_rec_fwd(h->stream, boff(Hall, (int64_t)(s - 1) * B * ldH, h->esz), ldH, Wh, G,
                                           Call + (int64_t)(s - 1) * B * H, B, H, boff(acts, (int64_t)s * B * ld4H, h->esz), ld4H,
                                           Call + (int64_t)s * B * H, boff(Hall, (int64_t)s * B * ldH, h->esz), h->zero_page, alone);
        if (e != hipSuccess) FAIL(h, LRCN_EHIP, "lstm_rec_fwd: %s", hipGetErrorString(e));
        return LRCN_OK;
    }
    if (s > 0)
        if (int rg = gemm(boff(Hall, (int64_t)(s - 1) * B * ldH, h->esz), ldH, Wh, ldH, G, 4 * H, B, 4 * H, H, true, false)) return rg;
    k_lstm_fwd(h->stream, h->dt, G, 4 * H, s ? Call + (int64_t)(s - 1) * B * H : nullptr, B, H,
               boff(acts, (int64_t)s * B * ld4H, h->esz), ld4H, Call + (int64_t)s * B * H,
               boff(Hall, (int64_t)s * B * ldH, h->esz), ldH, nullptr);
    return LRCN_OK;
}

template <class Handle, class Gemm>
int lstm_recurrence_fwd(Handle *h, bool alone, const Gemm &gemm, int S, int B, int H, int64_t ldH, int64_t ld4H, float *Gx, const void *Wh,
                        void *acts, float *Call, void *Hall) {
    const bool fused = lstm_fused_on(h->dt, B, H, ldH, ld4H);
    for (int s = 0; s < S; ++s)
        if (int r = lstm_step_fwd(h, alone, gemm, fused, s, B, H, ldH, ld4H, Gx, Wh, acts, Call, Hall)) return r;
    return LRCN_OK;
}

// The reverse recurrence of the same layer: dHall f32 [S*B][H] (external dh per step) -> dZ (T) [S*B][ld4H]; WhT (T) [H][ld4H].
template <class Handle, class Gemm>
int lstm_recurrence_bwd(Handle *h, bool alone, const Gemm &gemm, int S, int B, int H, int64_t ld4H, const void *acts, const float *Call,
                        const float *dHall, const void *WhT, void *dZ) {
    const int dt = h->dt;
    if (lstm_fused_on(dt, B, H, ld64(H), ld4H)) {
        // cell backward of the last step, then one launch per step: dh_rec = dZ[s] Wh fused with the cell backward of s-1
        k_lstm_bwd(h->stream, dt, boff(acts, (int64_t)(S - 1) * B * ld4H, h->esz), ld4H, S > 1 ? Call + (int64_t)(S - 2) * B * H : nullptr,
                   Call + (int64_t)(S - 1) * B * H, dHall + (int64_t)(S - 1) * B * H, H, nullptr, 0, h->dc, 1, B, H,
                   boff(dZ, (int64_t)(S - 1) * B * ld4H, h->esz), ld4H);
        for (int s = S - 1; s >= 1; --s) {
            hipError_t e = launch_lstm_rec_bwd(h->stream, boff(dZ, (int64_t)s * B * ld4H, h->esz), ld4H, WhT,
                                               boff(acts, (int64_t)(s - 1) * B * ld4H, h->esz), s > 1 ? Call + (int64_t)(s - 2) * B * H : nullptr,
                                               Call + (int64_t)(s - 1) * B * H, dHall + (int64_t)(s - 1) * B * H, h->dc, B, H,
                                               boff(dZ, (int64_t)(s - 1) * B * ld4H, h->esz), h->zero_page, alone);
            if (e != hipSuccess) FAIL(h, LRCN_EHIP, "lstm_rec_bwd: %s", hipGetErrorString(e));
        }
        return LRCN_OK;
    }
    for (int s = S - 1; s >= 0; --s) {
        k_lstm_bwd(h->stream, dt, boff(acts, (int64_t)s * B * ld4H, h->esz), ld4H, s ? Call + (int64_t)(s - 1) * B * H : nullptr,
                   Call + (int64_t)s * B * H, dHall + (int64_t)s * B * H, H, h->dhrec, s < S - 1, h->dc, s == S - 1, B, H,
                   boff(dZ, (int64_t)s * B * ld4H, h->esz), ld4H);
        if (s > 0)  // dh_prev = dZ[s] * Wh'   (Wh' K-contiguous = WhT [H][ld4H]); dhrec was zeroed by the cell kernel above
            if (int rg = gemm(boff(dZ, (int64_t)s * B * ld4H, h->esz), ld4H, WhT, ld4H, h->dhrec, H, B, H, 4 * H, false, true)) return rg;
    }
    return LRCN_OK;
}

}  // namespace lrcn_impl
