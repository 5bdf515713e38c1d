"""GPU: a context that was made for the largest batch and has already been used gives, bit for bit, what a fresh context of exactly the call's
size gives -- the regime dp.py, the trainer and the CLI run in (one context, then short last batches, variable T, decodes of any N * K, and
the step after a skipped non-finite step), and which rests on invariants the sources only state in comments: K-padding that holds zeros or
stale-but-finite values meeting a zero, an embedding staging array that is all zero on entry and exit, transposed operands re-viewed with
another leading dimension every call, dc / dhrec and the log-likelihood accumulator re-initialised by their own kernels.

1. eight lossgradient calls of other sizes on one (max_B = 300, max_T = 11) context, LRCN_OPT_DETERMINISTIC: loss `==` and all nine
   gradients as bytes against a fresh exact-size context, bf16 / f32, two layers / LRCN-1f; once in the float-atomic mode against the
   bf16-emulating oracle (parity_util's own constants).
2. a train_step whose features and parameters hold NaN (loss NaN, every gradient non-finite, the update skipped), then clean steps: all
   finite, and with the ordered sums bit-identical to the same steps on fresh contexts that never saw the NaN.  Nothing on the training path
   turns a float into an address (only token ids index memory), so the NaN can only show up as a value.
3. decodes after a larger decode (finite values only: a NaN logit could become a token id), 4. the activity handle.

A stale element that the current call did not write and that meets no written zero cannot sit under a bit comparison and cannot survive a NaN.
(Measured once with transpose_multi_kernel's zero fill of [R + shift, ld_dst) taken out: call 2 of part 1 is then off by 3e-4 of the largest
gradient element in W1, W2, Wproj and Wout -- inside parity_util's bounds, red here -- every recovery step of part 2 returns 240000 NaN in
dW1, and the T = 0 call and the activity handle go red as well; the decodes, which transpose nothing, stay green.)
Nothing here depends on the route a call takes: the fresh context takes the same one (the router sees M, N, K, never max_B / max_T).
"""
import functools
import math

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import activity as A
from lrcn_amd import lrcn as L
from oracle import oracle as orc
from parity_util import BF16_LOSS_RTOL, assert_bf16_matches_emulation, emulated_reference

import dropout_ref as dr
import torch_ref as tr
import varlen_ref as vr

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16

# ld64(E) = 128, ld64(H) = 256, ld64(V) = 1024, ld64(4H) = 832, LRCN-1f: ld64(E + h) = 256: every leading dimension has real padding
E, H, V = 100, 200, 1003
MAX_B, MAX_T = 300, 11
PDROP = 0.4
GCLIP = 5.0

# (B, T) of the calls, in order.  1: fills every scratch buffer to its end, GEMM + cell route.  2: M = 259, ldM = 320, fused small-batch
# route.  3: T = 0, the zero-filled h_prev block, M below one tile.  4: the four-row-block fused form.  5: mixed lens (0, 1 and T).
# 6: long T, small B.  7: back to the full batch.  8: call 2's inputs again.
CALLS = ((300, 11), (37, 6), (5, 0), (128, 2), (160, 3), (24, 11), (300, 1), (37, 6))
VARLEN = 4            # index of the mixed-length call
ORACLE_CALLS = (1, 2, 5)   # indices of calls 2, 3 and 6: held to the emulating oracle in the float-atomic mode
RECOVERY = (1, 2, 4, 0)    # the clean steps after the poisoned one: (37, 6), (5, 0), (160, 3) with mixed lens, (300, 11)


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def model(n_layers=2):
    m = orc.init_weights(E, H, H, V, seed=11, n_layers=n_layers)
    for n in ("W1", "W2", "Wout", "Wproj"):   # gates away from the linear regime, as test_recurrence_kernel_routes_by_batch_size_vs_oracle_bf16
        if m.p[n].size:
            m.p[n] *= 2.0
    return m


@functools.lru_cache(maxsize=None)
def call_inputs(k):
    """Call k's own seeded features, tokens and dropout seed (and lens / norm_tokens for the mixed-length call)."""
    if k == 7:
        return call_inputs(1)
    B, T = CALLS[k]
    rng = np.random.default_rng(500 + k)
    c = Inputs()
    c.B, c.T = B, T
    c.feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    c.tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    c.seed = 0x5EED0000 + k
    c.lens = c.norm_tokens = None
    if k == VARLEN:
        # lengths 0, 1 and T = 3 only, and a global token count (about twice this batch's) that is a multiple of every len + 1: the
        # emulating oracle of tests/varlen_ref.py then rounds d(logits) at the library's own scale
        c.lens = rng.choice([0, 1, T], size=B).astype(np.int32)
        c.lens[:3] = (0, 1, T)
        c.norm_tokens = 2 * vr.norm_tokens_of(c.lens)
        c.norm_tokens += -c.norm_tokens % 4
        assert vr.integer_row_norms(c.lens, c.norm_tokens) is not None
    return c


def make_ctx(max_B, max_T, dtype, n_layers=2, det=True, fused=False):
    ctx = L.Context(E, H, H, V, max_B=max_B, max_T=max_T, lstm_dtype=dtype, n_layers=n_layers)
    ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1 if det else 0)
    ctx.set_option(_lib.LRCN_OPT_FUSED_UPDATE, 1 if fused else 0)
    return ctx


def download(tensors):
    torch.cuda.synchronize()
    return [L.from_jl(t).copy() for t in tensors]


def run_call(ctx, param, k):
    c = call_inputs(k)
    grads, val = L.lossgradient(ctx, param, L.to_jl(c.feats), c.tokens, pdrop=PDROP, seed=c.seed, lens=c.lens, norm_tokens=c.norm_tokens)
    return val, download(grads)


@functools.lru_cache(maxsize=None)
def fresh_call(k, dtype, n_layers):
    """Call k on a context created for exactly that call (ordered sums), computed once per process."""
    B, T = CALLS[k]
    ctx = make_ctx(B, max(T, 1), dtype, n_layers)
    try:
        return run_call(ctx, L.model_from_arrays(model(n_layers).p), k)
    finally:
        ctx.close()


def differences(what, got, want, names=orc.PARAM_NAMES):
    """The places where (loss, arrays) `got` is not `want` to the bit, as one line each."""
    out = []
    if not got[0] == want[0]:
        out.append("%s: loss %r, expected %r" % (what, got[0], want[0]))
    for n, a, b in zip(names, got[1], want[1]):
        assert a.shape == b.shape, (what, n, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            ne = ~((a == b) | (np.isnan(a) & np.isnan(b)))
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            out.append("%s: %s differs in %d of %d elements (%d non-finite), max |d| %.3e at max |expected| %.3e" % (
                what, n, int(ne.sum()), a.size, int((~np.isfinite(a)).sum()), np.nanmax(d) if d.size else 0.0, np.abs(b).max()))
    return out


def all_finite(arrays):
    return all(np.isfinite(a).all() for a in arrays)


# ---------------------------------------------------------------------------------------------- 1. call sequences
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("dtype", [BF16, F32])
def test_loss_gradient_calls_of_other_sizes_on_a_used_context_equal_fresh_contexts(dtype, n_layers):
    ctx = make_ctx(MAX_B, MAX_T, dtype, n_layers)
    try:
        param = L.model_from_arrays(model(n_layers).p)
        got = [run_call(ctx, param, k) for k in range(len(CALLS))]
    finally:
        ctx.close()
    bad = []
    for k, (B, T) in enumerate(CALLS):
        assert math.isfinite(got[k][0]) and all_finite(got[k][1]), k
        bad += differences("call %d (B=%d, T=%d)" % (k + 1, B, T), got[k], fresh_call(k, dtype, n_layers))
    bad += differences("call 8 against call 2", got[7], got[1])
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def oracle_call(k):
    """The bf16-emulating oracle (and, as `.f32`, the plain one) on call k, the device's dropout masks from their host transcription."""
    c = call_inputs(k)
    mask1, mask2 = dr.masks(c.seed, PDROP, c.T, c.B, E, H)
    return emulated_reference(model(), c.feats, c.tokens, mask1=mask1, mask2=mask2)


def test_float_atomic_calls_on_a_used_context_match_the_emulating_oracle_bf16():
    ctx = make_ctx(MAX_B, MAX_T, BF16, det=False)
    try:
        param = L.model_from_arrays(model().p)
        got = [run_call(ctx, param, k) for k in range(len(CALLS))]
    finally:
        ctx.close()
    for k in ORACLE_CALLS:
        emu_loss, emu_g = oracle_call(k)
        assert_bf16_matches_emulation(got[k][0], got[k][1], emu_loss, emu_g, "call %d (B=%d, T=%d) after larger calls" % ((k + 1,) + CALLS[k]))


# ---------------------------------------------------------------------------------------------- 2. the step after a non-finite step
@functools.lru_cache(maxsize=None)
def poison():
    """Call 1's batch with a NaN in every feature row, and the model with a NaN in every tensor.  (Both: the features enter at LSTM-2 only.)"""
    c = call_inputs(0)
    feats = c.feats.copy()
    feats[np.arange(c.B), (np.arange(c.B) * 37) % 4096] = np.nan
    p = {n: a.copy() for n, a in model().p.items()}
    for a in p.values():
        a.reshape(-1)[a.size // 3] = np.nan
    return feats, p


@functools.lru_cache(maxsize=None)
def start_moments():
    rng = np.random.default_rng(77)
    shapes = [model().p[n].shape for n in orc.PARAM_NAMES]
    return ([(rng.standard_normal(s) * 0.01).astype(np.float32) for s in shapes],
            [(rng.standard_normal(s) ** 2 * 1e-4).astype(np.float32) for s in shapes])


START_T = 3   # Adam steps behind the run when it begins


def start_state(param_arrays):
    param = L.model_from_arrays(param_arrays)
    optim = L.initparams(param)
    m, v = start_moments()
    optim.m, optim.v, optim.t = L.model_from_arrays(m), L.model_from_arrays(v), START_T
    return param, optim, L.zeros_like_model(param)


def clean_step(ctx, param, optim, grads, k):
    c = call_inputs(k)
    val = L.train_step(ctx, param, optim, grads, L.to_jl(c.feats), c.tokens, pdrop=PDROP, seed=c.seed, want_loss=True, lens=c.lens,
                       norm_tokens=c.norm_tokens, gclip=GCLIP)
    return val, download(grads) + download(param) + download(optim.m) + download(optim.v)


STATE_NAMES = tuple("%s %s" % (w, n) for w in ("gradient", "parameter", "m", "v") for n in orc.PARAM_NAMES)


@functools.lru_cache(maxsize=None)
def unpoisoned_steps(fused):
    """The recovery steps from the same start, each on a fresh exact-size context that never saw a NaN (ordered sums)."""
    param, optim, grads = start_state(model().p)
    optim.t += 1   # the poisoned step advanced the caller's step counter
    out = []
    for k in RECOVERY:
        B, T = CALLS[k]
        ctx = make_ctx(B, max(T, 1), BF16, det=True, fused=fused)
        try:
            out.append(clean_step(ctx, param, optim, grads, k))
        finally:
            ctx.close()
    return out


def emulated_loss(param_arrays, k):
    """The emulating oracle's loss of call k at the given parameters."""
    c = call_inputs(k)
    m = orc.init_weights(E, H, H, V, seed=11)
    for n, a in zip(orc.PARAM_NAMES, param_arrays):
        m.p[n][...] = a
    mask1, mask2 = dr.masks(c.seed, PDROP, c.T, c.B, E, H)
    with orc.emulate_bf16():
        if c.lens is not None:
            return vr.loss(m, c.feats, c.tokens, c.lens, c.norm_tokens, mask1=mask1, mask2=mask2, row_norms=vr.integer_row_norms(c.lens, c.norm_tokens))
        return orc.loss(m, c.feats, c.tokens, mask1=mask1, mask2=mask2)


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("fused", [False, True])
def test_clean_steps_after_a_skipped_non_finite_step_equal_steps_that_never_saw_it(fused, det):
    bad_feats, bad_p = poison()
    c0 = call_inputs(0)
    ctx = make_ctx(MAX_B, MAX_T, BF16, det=det, fused=fused)
    try:
        bad_param, optim, grads = start_state(bad_p)
        before = download(bad_param) + download(optim.m) + download(optim.v)
        ctx.params_touched()
        val = L.train_step(ctx, bad_param, optim, grads, L.to_jl(bad_feats), c0.tokens, pdrop=PDROP, seed=99, want_loss=True, gclip=GCLIP)
        # the poison took ...
        assert math.isnan(val), val
        for n, g in zip(orc.PARAM_NAMES, download(grads)):
            assert not np.isfinite(g).all(), "the NaN did not reach the gradient of %s" % n
        st = L.clip_stats(ctx)
        assert st["skipped"] == 1 and st["last_skipped"] == 1 and st["steps"] == 1, st
        # ... and the skip contract held
        after = download(bad_param) + download(optim.m) + download(optim.v)
        assert [a.tobytes() for a in after] == [b.tobytes() for b in before]
        assert optim.t == START_T + 1
        # recovery on the clean set
        param = L.model_from_arrays(model().p)
        ctx.params_touched()
        got, params_before = [], []
        for k in RECOVERY:
            if not det:
                params_before.append(download(param))
            got.append(clean_step(ctx, param, optim, grads, k))
        st = L.clip_stats(ctx)
    finally:
        ctx.close()
    bad = []
    for i, k in enumerate(RECOVERY):
        what = "step %d (B=%d, T=%d) after the skipped one" % ((i + 1,) + CALLS[k])
        assert math.isfinite(got[i][0]), (what, got[i][0])
        for n, a in zip(STATE_NAMES, got[i][1]):
            assert np.isfinite(a).all(), "%s: %s holds %d non-finite values" % (what, n, int((~np.isfinite(a)).sum()))
        if det:
            bad += differences(what, got[i], unpoisoned_steps(fused)[i], STATE_NAMES)
        elif i == 0:   # the first step runs at the start parameters: the oracle reference of part 1's call 2
            emu_loss, emu_g = oracle_call(k)
            assert_bf16_matches_emulation(got[i][0], got[i][1][:9], emu_loss, emu_g, what)
        else:   # later steps: the loss at the parameters as they were before the step
            ref = emulated_loss(params_before[i], k)
            assert abs(got[i][0] - ref) <= BF16_LOSS_RTOL * abs(ref), (what, got[i][0], ref)
    assert not bad, "\n".join(bad)
    assert st["skipped"] == 1 and st["steps"] == 1 + len(RECOVERY) and st["last_skipped"] == 0, st


def test_loss_gradient_after_a_non_finite_call_equals_fresh_contexts_f32():
    """The same through lossgradient alone: the forward and backward scratch without the update kernels."""
    bad_feats, bad_p = poison()
    c0 = call_inputs(0)
    ctx = make_ctx(MAX_B, MAX_T, F32)
    try:
        g, val = L.lossgradient(ctx, L.model_from_arrays(bad_p), L.to_jl(bad_feats), c0.tokens, pdrop=PDROP, seed=99)
        assert math.isnan(val), val
        for n, a in zip(orc.PARAM_NAMES, download(g)):
            assert not np.isfinite(a).all(), "the NaN did not reach the gradient of %s" % n
        param = L.model_from_arrays(model().p)
        got = [run_call(ctx, param, k) for k in RECOVERY]
    finally:
        ctx.close()
    bad = []
    for i, k in enumerate(RECOVERY):
        what = "call %d (B=%d, T=%d) after the non-finite one" % ((i + 1,) + CALLS[k])
        assert math.isfinite(got[i][0]) and all_finite(got[i][1]), what
        bad += differences(what, got[i], fresh_call(k, F32, 2))
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------- 3. decode after a larger decode
DEC_MAX_B, DEC_MAX_T, NWORD = 320, 4, 8
# (kind, N, K or samples); the last repeats the first
DECODES = (("beam", 64, 5), ("beam", 3, 5), ("beam", 10, 32), ("sample", 7, 4), ("nbest", 9, 6), ("lossgrad", 20, 4), ("beam", 64, 5))
# The seed of the decodes' features: the best of 40 tried.  The model is close to a uniform softmax, so a beam's first two hypotheses lie
# within ~1e-5 of each other at most seeds; TIE_MARGIN is 20 times what nine float32 multiplications and a float32 softmax can move a
# probability by (9 * 2^-24 = 5.4e-7), so under float32 no two orders can differ by rounding.  (Both contexts run the same arithmetic on the
# same inputs in either precision; an exact tie is what would leave the order to something else.)
DECODE_SEED, TIE_MARGIN = 15, 1.0 + 1e-5


def decode_feats(i):
    i = 0 if i == 6 else i
    return (np.random.default_rng(DECODE_SEED * 100 + i).standard_normal((DECODES[i][1], 4096)) * 0.05).astype(np.float32)


def f32_bytes(values):
    return np.asarray(values, np.float32).tobytes()


def run_decode(ctx, param, i):
    kind, N, K = DECODES[i]
    feats = L.to_jl(decode_feats(i))
    if kind == "beam":
        out = L.beam_search_batch(ctx, param, feats, K, NWORD)
        return [t for t, _ in out], f32_bytes([p for _, p in out])
    if kind == "sample":
        out = L.sample_batch(ctx, param, feats, K, NWORD, top_k=40, top_p=0.9, seed=4242)
        return [[t for t, _ in img] for img in out], f32_bytes([lp for img in out for _, lp in img])
    if kind == "nbest":
        out = L.beam_nbest_batch(ctx, param, feats, K, NWORD, alpha=0.7)
        return [[t for t, _, _ in img] for img in out], f32_bytes([lp for img in out for _, lp, _ in img]), f32_bytes([s for img in out for _, _, s in img])
    tokens = np.random.default_rng(900 + i).integers(3, V, size=(K, N)).astype(np.int32)   # "lossgrad": B = N, T = K
    grads, val = L.lossgradient(ctx, param, feats, tokens, pdrop=PDROP, seed=31)
    return val, [a.tobytes() for a in download(grads)]


def test_decode_inputs_have_no_tied_hypotheses():
    """CPU: tests/torch_ref.py's float64 beam on every image of the three beam calls, winner over runner-up (as production_width.beam_reference)."""
    p = {n: torch.tensor(model().p[n], dtype=torch.float64) for n in orc.PARAM_NAMES}
    worst = math.inf
    for i in (0, 1, 2):
        for f in decode_feats(i):
            xs = tr.beam_search_ref(p, torch.tensor(f[None], dtype=torch.float64), DECODES[i][2], NWORD)
            worst = min(worst, float(xs[0][1]) / float(xs[1][1]))
    print("smallest winner / runner-up ratio: %.9f" % worst)
    assert worst >= TIE_MARGIN, worst


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_decodes_after_a_larger_decode_equal_fresh_contexts(dtype):
    def ctx_for(max_B):
        return make_ctx(max_B, DEC_MAX_T, dtype)   # ordered sums: the lossgradient call between the decodes is compared as bytes
    param = L.model_from_arrays(model().p)
    ctx = ctx_for(DEC_MAX_B)
    try:
        got = [run_decode(ctx, param, i) for i in range(len(DECODES))]
    finally:
        ctx.close()
    assert got[6] == got[0], "the first decode again, after six other calls"
    assert max(len(t) for t in got[0][0]) > 2   # captions, not just [bos, eos]
    for i, (kind, N, K) in enumerate(DECODES[:6]):
        fresh = ctx_for(N if kind == "lossgrad" else N * K)
        try:
            want = run_decode(fresh, param, i)
        finally:
            fresh.close()
        assert got[i] == want, "call %d: %s N=%d K=%d" % (i + 1, kind, N, K)


# ---------------------------------------------------------------------------------------------- 4. activity handle
ACT_F, ACT_H, ACT_C, ACT_MAX_B, ACT_MAX_T = 192, 200, 11, 96, 12
ACT_CALLS = ((96, 12, False), (5, 3, False), (33, 12, True), (96, 1, False), (5, 3, False))   # (B, T, mixed lens); the last repeats the second


def run_activity(m, params, i):
    i = 1 if i == 4 else i
    B, T, mixed = ACT_CALLS[i]
    rng = np.random.default_rng(300 + i)
    x = rng.standard_normal((B * T, ACT_F)).astype(np.float32)
    lab = rng.integers(0, ACT_C, B).astype(np.int32)
    lens = None
    if mixed:
        lens = rng.integers(1, T + 1, B).astype(np.int32)
        lens[0], lens[-1] = 1, T
    loss = m.loss_grad(x, lab, lens, T, params=params)
    g = download(m.grads)
    cp, fp = m.predict(x, lens, T, B=B, frame_probs=True, params=params)
    return loss, g + download([cp, fp])


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_activity_calls_of_other_sizes_on_a_used_handle_equal_fresh_handles(dtype):
    names = A.PARAM_NAMES + ("clip probabilities", "frame probabilities")
    m = A.ActivityModel(ACT_F, ACT_H, ACT_C, max_B=ACT_MAX_B, max_T=ACT_MAX_T, dtype=dtype, deterministic=True, seed=7)
    try:
        got = [run_activity(m, m.params, i) for i in range(len(ACT_CALLS))]
        bad = differences("call 5 against call 2", got[4], got[1], names)
        for i, (B, T, _) in enumerate(ACT_CALLS[:4]):
            assert math.isfinite(got[i][0]) and all_finite(got[i][1]), i
            fresh = A.ActivityModel(ACT_F, ACT_H, ACT_C, max_B=B, max_T=T, dtype=dtype, deterministic=True, seed=None)
            try:
                bad += differences("call %d (B=%d, T=%d)" % (i + 1, B, T), got[i], run_activity(fresh, m.params, i), names)
            finally:
                fresh.close()
    finally:
        m.close()
    assert not bad, "\n".join(bad)
