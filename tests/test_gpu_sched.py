"""GPU: scheduled sampling in caption training (include/lrcn_sched.h) against tests/sched_ref.py.

The chain is pinned step by step, never against an end-to-end simulation (two chains may part ways at a near tie): every coin is checked
exactly; every draw is checked against the host draw from the DEVICE's logits row of the step before (logits_out); loss, gradients and
logits are checked against the float64 autograd reference under the DEVICE's fed words (fed_out).

Tolerances are the project's own: f32 loss 1e-5 relative, gradients rtol 1e-3 + atol 1e-5 (tests/test_gpu_varlen.py), logits rtol 1e-4 +
atol 2e-5 (tests/test_gpu_lstm_parity.py's forward-logits parity), bf16 the independent bound of tests/parity_util.py.  A draw may differ
from the host's only where nucleus_ref.excused allows (top two scores within 1e-4 (1 + |best|): the device's logf), for at most 2 % of at
least 200 draws per case; at temperature 0 nothing is excused."""
import ctypes as C

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L
from oracle import oracle as orc
from parity_util import assert_bf16_near_f32_oracle

import nucleus_ref as nr
import sched_ref as sr
import varlen_ref as vr

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
NO_COIN = 1e-9   # below the smallest u (2^-24): the stepwise route with no coin firing


def make(seed, B, T, E, H, V, dtype, n_layers=2, det=False):
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed + 1, n_layers=n_layers)
    feats = (rng.standard_normal((B, 4096)) * 0.02).astype(np.float32)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    ctx = L.Context(E, H, H, V, max_B=B, max_T=max(T, 1), lstm_dtype=dtype, n_layers=n_layers)
    if det:
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    return rng, m, feats, tokens, ctx, L.model_from_arrays(m.p)


def masks_for(rng, n_layers, T, B, E, H):
    kw = {"mask1": ((rng.random((T + 1, B, E if n_layers == 2 else E + H // 2)) > 0.4) / 0.6).astype(np.float32)}
    if n_layers == 2:
        kw["mask2"] = ((rng.random((T + 1, B, H)) > 0.4) / 0.6).astype(np.float32)
    return kw


def host(grads):
    return [L.from_jl(g).copy() for g in grads]


def grads_close_f32(got, ref_g, what=""):
    for n, g in zip(orc.PARAM_NAMES, got):
        if ref_g.p[n].size:
            np.testing.assert_allclose(g if isinstance(g, np.ndarray) else L.from_jl(g), ref_g.p[n], rtol=1e-3, atol=1e-5, err_msg="%s %s" % (what, n))


def same_bits(a, b, what=""):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "%s: tensor %d differs" % (what, k)


# ------------------------------------------------------------------------------------------------ 1. exports
def test_the_four_exports_exist():
    lib = C.CDLL(_lib.LIB_PATH)
    names = {"lrcn_loss_sched", "lrcn_loss_grad_sched", "lrcn_train_step_sched", "lrcn_sched_stats"}
    for n in names:
        assert hasattr(lib, n), n
    assert set(_lib.SCHED_SIGNATURES) == names
    assert lib.lrcn_abi_version() == 5


# ------------------------------------------------------------------------------------------------ 2. eps = 0
@pytest.mark.parametrize("pdrop", [0.0, 0.4])
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_eps0_is_bit_identical_to_the_time_batched_calls(dtype, n_layers, pdrop):
    B, T, E, H, V = 24, 6, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(11, B, T, E, H, V, dtype, n_layers, det=True)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    w = rng.uniform(-1, 2, size=B).astype(np.float32)
    f = L.to_jl(feats)
    for kw in ({}, {"row_weights": w}):
        ga, la = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=150, **kw)
        ga = host(ga)
        gb, lb, fed = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=150, sched=(0.0, 1.0, 5), return_fed=True, **kw)
        assert la == lb and L.last_loss(ctx) == lb
        same_bits(ga, host(gb), "eps 0")
        assert np.array_equal(fed, sr.gold_inputs(tokens, lens))
        assert L.sched_stats(ctx) == (int(lens.sum()), 0)
        assert L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=150, sched=(0.0, 0.0, 5), **kw) == \
            L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=150, **kw)
        assert any(np.abs(a).max() > 0 for a in ga)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the stepwise route, no coin firing
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("n_layers,B,T,E,H,V", [(2, 13, 7, 52, 36, 97), (1, 11, 6, 40, 48, 203)])
def test_stepwise_route_without_draws_f32_vs_oracle(n_layers, B, T, E, H, V, masks):
    rng, m, feats, tokens, ctx, param = make(B + T, B, T, E, H, V, F32, n_layers)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    kw = masks_for(rng, n_layers, T, B, E, H) if masks else {}
    ref, ref_g = vr.loss(m, feats, tokens, lens, None, want_grad=True, **kw)
    for _ in range(2):   # twice: scratch carries the first pass's values
        g, val, fed = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, sched=(NO_COIN, 1.0, 3), return_fed=True, **kw)
        print("stepwise f32: loss", val, "ref", ref, "rel", abs(val - ref) / abs(ref))
        assert np.array_equal(fed, sr.gold_inputs(tokens, lens))
        assert L.sched_stats(ctx) == (int(lens.sum()), 0)
        assert abs(val - ref) <= 1e-5 * abs(ref)
        grads_close_f32(g, ref_g)
    only = L.loss(ctx, param, L.to_jl(feats), tokens, lens=lens, sched=(NO_COIN, 1.0, 3), **kw)
    assert abs(only - ref) <= 1e-5 * abs(ref)
    ctx.close()


@pytest.mark.parametrize("n_layers,B,T,E,H,V", [(2, 13, 7, 52, 36, 97), (1, 11, 6, 40, 48, 203)])
def test_stepwise_route_applies_the_seeded_dropout_of_every_step(n_layers, B, T, E, H, V):
    # the masks of a seeded dropout are functions of (step, row, column): a launch that restarted at step 0 would not match the backward's
    rng, m, feats, tokens, ctx, param = make(B, B, T, E, H, V, F32, n_layers)
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    f = L.to_jl(feats)
    ga, la = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=17, lens=lens)
    ga = host(ga)
    gb, lb = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=17, lens=lens, sched=(NO_COIN, 1.0, 3))
    print("seeded dropout: stepwise", lb, "time-batched", la)
    assert abs(la - lb) <= 1e-5 * abs(la)
    for n, a, b in zip(orc.PARAM_NAMES, ga, host(gb)):
        np.testing.assert_allclose(b, a, rtol=1e-3, atol=1e-5, err_msg=n)
    ctx.close()


@pytest.mark.parametrize("B", [256, 48])
def test_stepwise_route_without_draws_bf16(B):
    # 256 rows: GEMM + cell kernel per recurrence step; 48 rows: the fused step kernels
    T, E, H, V = 5, 64, 64, 157
    rng, m, feats, tokens, ctx, param = make(B, B, T, E, H, V, BF16)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    f32_loss, f32_g = vr.loss(m, feats, tokens, lens, want_grad=True)
    g, val, fed = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, sched=(NO_COIN, 1.0, 3), return_fed=True)
    print("stepwise bf16 B=%d: loss" % B, val, "f32", f32_loss)
    assert np.array_equal(fed, sr.gold_inputs(tokens, lens))
    assert_bf16_near_f32_oracle(val, g, f32_loss, f32_g, "sched bf16 B=%d" % B)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. coins and draws
@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_every_coin_and_every_draw_from_the_device_logits(name):
    """The V = 15360 | 15361 cases sit on both sides of k_sched_next_input's `stage` flag, bf16-V16400 runs its unstaged form in bf16; their
    models give the last word a quarter of every row (sched_ref.LAST_COLUMN_CASES).  A local build (not kept) whose staged copy lost its
    last element (row_max_stage read it as -inf) failed every staged case -- [f32-V15360-eps1-t1] at its first call (word 7777 drawn for
    the host's 15359) -- and passed the three unstaged ones."""
    dtype, nl, B, T, E, H, V, eps, temp, row0, mixed, calls = sr.CASES[name]
    m, feats, tokens, lens, seeds = sr.case_inputs(name)
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=BF16 if dtype == "bf16" else F32, n_layers=nl)
    param, f = L.model_from_arrays(m.p), L.to_jl(feats)
    gold = sr.gold_inputs(tokens, lens)
    draws = excused = 0
    for seed in seeds:
        g, val, fed, z = L.lossgradient(ctx, param, f, tokens, pdrop=0.3, seed=seed & 0xFFFF, lens=lens, sched=(eps, temp, seed, row0),
                                        return_fed=True, return_logits=True)
        fire = sr.coins(seed, eps, lens, T, row0)
        assert np.isfinite(val) and z.shape == (T + 1, B, V)
        assert np.array_equal(fed[~fire], gold[~fire]), "an input whose coin did not fire is not the gold word (or eos / bos)"
        for s, b in zip(*np.nonzero(fire)):
            cols, sc = sr.draw_scores(z[s - 1, b], temp, seed, row0 + int(b), int(s))
            want = int(cols[np.argmax(sc)])
            draws += 1
            if int(fed[s, b]) != want:
                assert temp > 0 and nr.excused(sc), (name, seed, s, b, int(fed[s, b]), want)
                assert sc[list(cols).index(int(fed[s, b]))] >= np.sort(sc)[-2], "the device's word is not one of the two tied columns"
                excused += 1
        assert L.sched_stats(ctx) == (int(lens.sum()), int(fire.sum()))
    print(name, "draws", draws, "excused", excused)
    assert draws >= sr.MIN_DRAWS
    assert excused <= sr.EXCUSED_SHARE * draws
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. gradients under the fed words
@pytest.mark.parametrize("eps", [1.0, 0.5])
@pytest.mark.parametrize("n_layers,B,T,E,H,V", [(2, 13, 7, 52, 36, 97), (1, 11, 6, 40, 48, 203)])
def test_loss_gradients_and_logits_under_the_fed_words_f32(n_layers, B, T, E, H, V, eps):
    rng, m, feats, tokens, ctx, param = make(3 * B, B, T, E, H, V, F32, n_layers)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    w = rng.uniform(-1, 2, size=B).astype(np.float32)
    kw = masks_for(rng, n_layers, T, B, E, H)
    for wkw, row_w in (({}, None), ({"row_weights": w}, w)):
        g, val, fed, z = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=77, sched=(eps, 1.0, 21, 500), return_fed=True,
                                        return_logits=True, **kw, **wkw)
        fire = sr.coins(21, eps, lens, T, 500)
        assert fire.sum() > 0 and (fed[fire] != sr.gold_inputs(tokens, lens)[fire]).any()
        ref_z = []
        ref, ref_g = sr.loss(m, feats, tokens, lens, fed, norm_tokens=77, row_w=row_w, want_grad=True, collect=ref_z, **kw)
        print("under fed words: loss", val, "ref", ref, "rel", abs(val - ref) / abs(ref), "drawn", int(fire.sum()))
        np.testing.assert_allclose(z, np.stack(ref_z), rtol=1e-4, atol=2e-5)
        assert abs(val - ref) <= 1e-5 * abs(ref)
        grads_close_f32(g, ref_g)
        # the embedding gradient lands on the fed words' rows: a word that was fed nowhere has a zero row
        unused = np.setdiff1d(np.arange(V), fed.ravel())
        assert unused.size and not np.abs(L.from_jl(g[orc.PARAM_NAMES.index("Wembed")])[unused]).any()
    ctx.close()


@pytest.mark.parametrize("eps", [1.0, 0.5])
@pytest.mark.parametrize("B,n_layers", [(256, 2), (48, 2), (48, 1)])
def test_loss_and_gradients_under_the_fed_words_bf16(B, n_layers, eps):
    T, E, H, V = 5, 64, 64, 157
    rng, m, feats, tokens, ctx, param = make(B + 1, B, T, E, H, V, BF16, n_layers)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    kw = masks_for(rng, n_layers, T, B, E, H)
    g, val, fed = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, sched=(eps, 1.0, 8), return_fed=True, **kw)
    ref, ref_g = sr.loss(m, feats, tokens, lens, fed, want_grad=True, **kw)
    print("bf16 under fed words B=%d: loss" % B, val, "f64", ref)
    assert_bf16_near_f32_oracle(val, g, ref, ref_g, "sched bf16 fed B=%d" % B)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. lengths and weights
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_lengths_padding_and_weights(dtype):
    B, T, E, H, V = 33, 8, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(21, B, T, E, H, V, dtype, det=True)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[3], lens[4] = T, 0
    f = L.to_jl(feats)
    ss = (0.5, 1.0, 77, 12)
    zeros = vr.pad_with(tokens, lens, 0)
    noise = vr.pad_with(tokens, lens, rng.integers(0, V, size=tokens.shape))
    assert (zeros != noise).any()
    ga, la, feda = L.lossgradient(ctx, param, f, zeros, lens=lens, pdrop=0.3, seed=4, sched=ss, return_fed=True)
    ga = host(ga)
    gb, lb, fedb = L.lossgradient(ctx, param, f, noise, lens=lens, pdrop=0.3, seed=4, sched=ss, return_fed=True)
    gb = host(gb)
    # steps past a row's end are fed eos, whatever the padding holds; the padding is never read, so it changes no bit
    for b in range(B):
        assert (feda[lens[b] + 1:, b] == 0).all() and feda[0, b] == 1
    assert la == lb and np.array_equal(feda, fedb)
    same_bits(ga, gb, "padding")
    # all weights 1.0: the bits of row_w = NULL
    gc, lc, fedc = L.lossgradient(ctx, param, f, zeros, lens=lens, pdrop=0.3, seed=4, sched=ss, return_fed=True, row_weights=np.ones(B, np.float32))
    assert lc == la and np.array_equal(fedc, feda)
    same_bits(ga, host(gc), "unit weights")
    # a zero-weight row still draws, and loss and gradients do not depend on its targets
    w = rng.uniform(0.5, 2, size=B).astype(np.float32)
    w[3] = 0.0
    gd, ld, fedd = L.lossgradient(ctx, param, f, zeros, lens=lens, pdrop=0.3, seed=4, sched=ss, return_fed=True, row_weights=w)
    gd = host(gd)
    fire = sr.coins(77, 0.5, lens, T, 12)
    assert fire[:, 3].any() and np.array_equal(fedd, feda)
    assert L.sched_stats(ctx) == (int(lens.sum()), int(fire.sum()))
    # (new targets for row 3 are new gold inputs too: wherever its coin does not fire the row is fed them -- but its d(logits) rows are zero
    # and rows do not mix, so it contributes exact zeros to every sum, before and after)
    other = zeros.copy()
    other[:, 3] = (other[:, 3] + 7) % (V - 3) + 3
    ge, le, fede = L.lossgradient(ctx, param, f, other, lens=lens, pdrop=0.3, seed=4, sched=ss, row_weights=w, return_fed=True)
    assert (fede[:, 3] != fedd[:, 3]).any() and np.array_equal(np.delete(fede, 3, 1), np.delete(fedd, 3, 1))
    assert le == ld
    same_bits(gd, host(ge), "zero-weight row")
    ctx.close()


def test_zero_weight_row_is_independent_of_its_targets_bitwise():
    # at eps = 1 every eligible input of the row is drawn, so its targets enter nowhere but the (zero-weighted) loss terms
    B, T, E, H, V = 9, 5, 24, 40, 131
    rng, m, feats, tokens, ctx, param = make(6, B, T, E, H, V, F32, det=True)
    lens = np.full(B, T, np.int32)
    w = np.ones(B, np.float32)
    w[2] = 0.0
    f = L.to_jl(feats)
    other = tokens.copy()
    other[:, 2] = (other[:, 2] + 7) % (V - 3) + 3
    ga, la, feda = L.lossgradient(ctx, param, f, tokens, lens=lens, sched=(1.0, 1.0, 3), row_weights=w, return_fed=True)
    ga = host(ga)
    gb, lb, fedb = L.lossgradient(ctx, param, f, other, lens=lens, sched=(1.0, 1.0, 3), row_weights=w, return_fed=True)
    assert la == lb and np.array_equal(feda, fedb) and (feda[1:, 2] != tokens[:, 2]).any()
    same_bits(ga, host(gb), "zero-weight row")
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. repeatability
@pytest.mark.parametrize("dtype,n_layers", [(F32, 2), (BF16, 2), (BF16, 1)])
def test_repeatable_on_a_deterministic_context_and_the_seed_matters(dtype, n_layers):
    B, T, E, H, V = 24, 6, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(12, B, T, E, H, V, dtype, n_layers, det=True)
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    f = L.to_jl(feats)
    ga, la, feda = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=2, lens=lens, sched=(0.5, 1.0, 99), return_fed=True)
    ga = host(ga)
    L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=2, lens=lens)   # (a time-batched call in between leaves no trace)
    gb, lb, fedb = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=2, lens=lens, sched=(0.5, 1.0, 99), return_fed=True)
    assert la == lb and np.array_equal(feda, fedb)
    same_bits(ga, host(gb), "repeat")
    _, _, fedc = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=2, lens=lens, sched=(0.5, 1.0, 100), return_fed=True)
    assert not np.array_equal(feda, fedc)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. train step
@pytest.mark.parametrize("gclip", [0.0, 0.05])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_train_step_sched_is_loss_grad_sched_then_adam(dtype, gclip):
    B, T, E, H, V = 16, 6, 64, 64, 211
    rng, m, feats, tokens, ctx, _ = make(31, B, T, E, H, V, dtype, det=True)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    w = rng.uniform(0.5, 2, size=B).astype(np.float32)
    f = L.to_jl(feats)
    res = []
    for fused in (True, False):
        param = L.model_from_arrays(m.p)
        optim = L.initparams(param)
        grads = [L.jl_empty(*t.shape) for t in param]
        losses = []
        for step in range(3):
            ss = (0.5, 1.0, 1000 + step, 3)
            kw = {"row_weights": w} if step == 2 else {}
            if fused:
                losses.append(L.train_step(ctx, param, optim, grads, f, tokens, pdrop=0.4, seed=step, want_loss=True, lens=lens, norm_tokens=200,
                                           gclip=gclip, sched=ss, **kw))
            else:
                _, val = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=step, grads=grads, lens=lens, norm_tokens=200, sched=ss, **kw)
                if gclip > 0:   # the clipped sequence of include/lrcn_clip.h
                    L.grad_sumsq(ctx, grads)
                    L.clip_set(ctx, gclip)
                L.update(ctx, param, grads, optim, clipped=gclip > 0)
                losses.append(val)
        res.append((losses, host(param), host(optim.m), optim.t))
    (la, pa, ma, ta), (lb, pb, mb, tb) = res
    assert la == lb and ta == tb == 3
    same_bits(pa + ma, pb + mb, "train step")
    if gclip > 0:
        assert L.clip_stats(ctx)["clipped"] > 0
    assert any(np.abs(a - L.from_jl(p0)).max() > 0 for a, p0 in zip(pa, L.model_from_arrays(m.p)) if a.size)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 9. rejection
def test_bad_arguments_return_einval_and_a_valid_call_still_works():
    B, T, E, H, V = 4, 3, 16, 16, 19
    rng, m, feats, tokens, ctx, param = make(2, B, T, E, H, V, F32)
    f, tok = L.to_jl(feats), torch.as_tensor(tokens).cuda()
    lib = _lib.lib()
    grads = [L.jl_empty(*t.shape) for t in param]
    out = C.c_double()
    ok = [3, 1, 0, 2]

    def call(lens=ok, w=None, ss=(0.5, 1.0, 1, 0), nt=10, T_=T, B_=B, drop=None, fe=f):
        la = np.asarray(lens, np.int32) if lens is not None else None
        lp = la.ctypes.data_as(C.POINTER(C.c_int32)) if la is not None else None
        wa = np.asarray(w, np.float32) if w is not None else None
        wp = wa.ctypes.data_as(C.POINTER(C.c_float)) if wa is not None else None
        s = _lib.Sched(*ss) if ss is not None else None
        sp = C.byref(s) if s is not None else None
        a = (ctx._h, L._p9(param), L._ptr(fe), C.c_void_p(tok.data_ptr()), lp, wp, T_, B_, C.c_int64(nt), drop, sp)
        return (lib.lrcn_loss_sched(*a, None, None, C.byref(out)), lib.lrcn_loss_grad_sched(*a, L._p9(grads), None, None, C.byref(out)),
                lib.lrcn_train_step_sched(ctx._h, L._p9(param), L._p9(grads), L._p9(grads), L._p9(grads), L._ptr(fe), C.c_void_p(tok.data_ptr()),
                                          lp, wp, T_, B_, C.c_int64(nt), drop, sp, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, C.byref(out)))

    EINVAL = (-1, -1, -1)
    nan, inf = float("nan"), float("inf")
    assert call(ss=None) == EINVAL
    assert call(ss=(nan, 1.0, 1, 0)) == EINVAL and call(ss=(-0.01, 1.0, 1, 0)) == EINVAL and call(ss=(1.01, 1.0, 1, 0)) == EINVAL
    assert b"eps" in lib.lrcn_last_error(ctx._h)
    assert call(ss=(0.5, nan, 1, 0)) == EINVAL and call(ss=(0.5, -1.0, 1, 0)) == EINVAL and call(ss=(0.5, inf, 1, 0)) == EINVAL
    assert call(ss=(0.5, 1.0, 1, -1)) == EINVAL and call(ss=(0.5, 1.0, 1, 2 ** 32 - B + 1)) == EINVAL
    assert call(ss=(0.0, 1.0, 1, -1)) == EINVAL   # (checked at eps 0 as well)
    assert call(lens=None) == EINVAL and b"lens" in lib.lrcn_last_error(ctx._h)
    # what lrcn_loss_grad_w rejects
    assert call(lens=[3, 1, 0, 4]) == EINVAL and call(lens=[3, -1, 0, 2]) == EINVAL and call(nt=0) == EINVAL
    assert call(w=[1.0, nan, 1.0, 1.0]) == EINVAL and call(w=[1.0, inf, 1.0, 1.0]) == EINVAL
    assert call(B_=0) == EINVAL and call(T_=-1) == EINVAL and call(T_=T + 1) == EINVAL and call(fe=None) == EINVAL
    bad_drop = _lib.Dropout(1.0, 0, None, None)
    assert call(drop=C.byref(bad_drop)) == EINVAL
    la = np.asarray(ok, np.int32)
    s = _lib.Sched(0.5, 1.0, 1, 0)
    assert lib.lrcn_loss_grad_sched(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), la.ctypes.data_as(C.POINTER(C.c_int32)), None, T, B,
                                    C.c_int64(10), None, C.byref(s), _lib.P9(*([None] * 9)), None, None, C.byref(out)) == -1
    ctx.sync()   # nothing was queued, nothing is pending
    # the largest admissible row0, and the context works afterwards
    g, val, fed = L.lossgradient(ctx, param, f, tokens, lens=ok, sched=(1.0, 1.0, 5, 2 ** 32 - B), return_fed=True)
    ref = sr.loss(m, feats, tokens, ok, fed)
    assert abs(val - ref) <= 1e-5 * abs(ref)
    with pytest.raises(lrcn_amd.LrcnError):
        L.lossgradient(ctx, param, f, tokens, lens=ok, return_fed=True)   # the wrapper's own check: return_fed needs sched
    ctx.close()
