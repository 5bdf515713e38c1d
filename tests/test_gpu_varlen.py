"""GPU: the variable-length caption loss, gradient and training step (include/lrcn_varlen.h) against tests/varlen_ref.py -- the
per-caption sums of the equal-length CPU oracle.

Tolerances are the ones the equal-length parity tests already use for lrcn_loss_grad: f32 loss 1e-5 relative, gradients rtol 1e-3 +
atol 1e-5 (tests/test_gpu_lstm_parity.py); bf16 the two bounds of tests/parity_util.py.  With every length equal to T and norm_tokens =
norm_B (T + 1) a deterministic context must return the bits of lrcn_loss_grad: the scale is the same float and no row is masked."""
import ctypes as C

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib, dp
from lrcn_amd import lrcn as L
from lrcn_amd import train as trn
from oracle import oracle as orc
from parity_util import assert_bf16_matches_emulation, assert_bf16_near_f32_oracle

import varlen_ref as vr

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16


def make(seed, B, T, E, H, V, dtype, n_layers=2, det=False, lens=None):
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed + 1, n_layers=n_layers)
    feats = (rng.standard_normal((B, 4096)) * 0.02).astype(np.float32)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    ctx = L.Context(E, H, H, V, max_B=B, max_T=max(T, 1), lstm_dtype=dtype, n_layers=n_layers)
    if det:
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    return rng, m, feats, tokens, ctx, L.model_from_arrays(m.p)


def host(grads):
    return [L.from_jl(g).copy() for g in grads]


def grads_close_f32(got, ref_g, what=""):
    for n, g in zip(orc.PARAM_NAMES, got):
        if ref_g.p[n].size:
            np.testing.assert_allclose(g if isinstance(g, np.ndarray) else L.from_jl(g), ref_g.p[n], rtol=1e-3, atol=1e-5, err_msg="%s %s" % (what, n))


def test_the_three_exports_exist():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("lrcn_loss_var", "lrcn_loss_grad_var", "lrcn_train_step_var"):
        assert hasattr(lib, n), n
    assert set(_lib.VARLEN_SIGNATURES) == {"lrcn_loss_var", "lrcn_loss_grad_var", "lrcn_train_step_var"}
    assert lib.lrcn_abi_version() == 5


@pytest.mark.parametrize("pdrop", [0.0, 0.4])
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_equal_lengths_are_bit_identical_to_loss_grad(dtype, n_layers, pdrop):
    B, T, E, H, V = 24, 6, 64, 64, 301
    for norm_B in (B, 4 * B):
        rng, m, feats, tokens, ctx, param = make(11, B, T, E, H, V, dtype, n_layers, det=True)
        f = L.to_jl(feats)
        ga, la = L.lossgradient(ctx, param, f, tokens, norm_B=norm_B, pdrop=pdrop, seed=9)
        ga = host(ga)
        lf = L.loss(ctx, param, f, tokens, norm_B=norm_B, pdrop=pdrop, seed=9)
        gb, lb = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=[T] * B, norm_tokens=norm_B * (T + 1))
        gb = host(gb)
        lg = L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=[T] * B, norm_tokens=norm_B * (T + 1))
        assert la == lb and lf == lg and L.last_loss(ctx) == lg
        for k, (a, b) in enumerate(zip(ga, gb)):
            assert np.array_equal(a, b), "gradient %d differs from lrcn_loss_grad's" % k
        assert any(np.abs(a).max() > 0 for a in ga)
        ctx.close()


@pytest.mark.parametrize("n_layers,masks,B,T,E,H,V", [(2, False, 13, 7, 52, 36, 97), (2, True, 9, 5, 24, 40, 131), (1, False, 11, 6, 40, 48, 203),
                                                      (1, True, 6, 4, 24, 32, 57), (2, False, 6, 3, 16, 16, 16400)])
def test_mixed_lengths_f32_vs_oracle(n_layers, masks, B, T, E, H, V):
    # V = 16400: the generic softmax kernel (above the register-resident form's 16384 columns)
    rng, m, feats, tokens, ctx, param = make(B + T, B, T, E, H, V, F32, n_layers)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    kw = {}
    if masks:
        kw["mask1"] = ((rng.random((T + 1, B, E if n_layers == 2 else E + H // 2)) > 0.4) / 0.6).astype(np.float32)
        if n_layers == 2:
            kw["mask2"] = ((rng.random((T + 1, B, H)) > 0.4) / 0.6).astype(np.float32)
    for nt in (None, 3 * vr.norm_tokens_of(lens)):   # the batch's own count, and a "global" one
        ref, ref_g = vr.loss(m, feats, tokens, lens, nt, want_grad=True, **kw)
        for _ in range(2):   # twice: scratch carries the first pass's values
            g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=nt, **kw)
            print("f32 mixed: loss", val, "ref", ref, "rel", abs(val - ref) / abs(ref))
            assert abs(val - ref) <= 1e-5 * abs(ref)
            grads_close_f32(g, ref_g)
        only = L.loss(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=nt, **kw)
        assert abs(only - ref) <= 1e-5 * abs(ref)
    ctx.close()


@pytest.mark.parametrize("B,n_layers", [(256, 2), (48, 2), (64, 1)])
def test_mixed_lengths_bf16_vs_emulating_oracle(B, n_layers):
    # >= 256 rows: GEMM + cell kernel per recurrence step; <= 64 rows: the fused step kernels.  Lengths such that norm_tokens / (len + 1) is an
    # integer for every row: the oracle's row b then rounds d(logits) at the library's scale 1 / norm_tokens.
    T, E, H, V = 5, 64, 64, 157
    rng, m, feats, tokens, ctx, param = make(B, B, T, E, H, V, BF16, n_layers)
    lens = vr.lens_with_integer_shares(B, rng)
    nb = vr.integer_row_norms(lens)
    assert nb is not None and lens.max() <= T
    ref, ref_g = vr.emulated_reference(m, feats, tokens, lens, row_norms=nb)
    g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens)
    print("bf16 mixed B=%d: loss" % B, val, "emulated", ref, "f32", ref_g.f32[0])
    assert_bf16_matches_emulation(val, g, ref, ref_g, "varlen bf16 B=%d" % B)
    ctx.close()


def test_arbitrary_lengths_bf16_vs_plain_oracle():
    B, T, E, H, V = 40, 9, 64, 64, 211
    rng, m, feats, tokens, ctx, param = make(5, B, T, E, H, V, BF16)
    lens = rng.integers(0, T, size=B).astype(np.int32)   # the longest caption is shorter than T: a whole padded step
    f32_loss, f32_g = vr.loss(m, feats, tokens, lens, want_grad=True)
    g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens)
    print("bf16 arbitrary: loss", val, "f32", f32_loss)
    assert_bf16_near_f32_oracle(val, g, f32_loss, f32_g, "varlen bf16 arbitrary lengths")
    ctx.close()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("det", [False, True])
def test_padding_content_does_not_matter(dtype, det):
    B, T, E, H, V = 33, 8, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(21, B, T, E, H, V, dtype, det=det)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[3] = T
    zeros = vr.pad_with(tokens, lens, 0)
    noise = vr.pad_with(tokens, lens, rng.integers(0, V, size=tokens.shape))
    assert (zeros != noise).any()
    f = L.to_jl(feats)
    ga, la = L.lossgradient(ctx, param, f, zeros, lens=lens, pdrop=0.3, seed=4)
    ga = host(ga)
    gb, lb = L.lossgradient(ctx, param, f, noise, lens=lens, pdrop=0.3, seed=4)
    gb = host(gb)
    assert la == lb
    if det:   # identical inputs repeat bit for bit; the padding is never read, so it is no input
        gc, lc = L.lossgradient(ctx, param, f, noise, lens=lens, pdrop=0.3, seed=4)
        assert lc == lb
        for a, b, c in zip(ga, gb, host(gc)):
            assert np.array_equal(b, c) and np.array_equal(a, b)
    # both against the oracle, without dropout
    f32_loss, f32_g = vr.loss(m, feats, tokens, lens, want_grad=True)
    for toks in (zeros, noise):
        g, val = L.lossgradient(ctx, param, f, toks, lens=lens)
        if dtype == F32:
            assert abs(val - f32_loss) <= 1e-5 * abs(f32_loss)
            grads_close_f32(g, f32_g)
        else:
            assert_bf16_near_f32_oracle(val, g, f32_loss, f32_g, "varlen padding")
    ctx.close()


def test_padding_cannot_raise_the_token_flag_and_active_ids_still_do():
    B, T, E, H, V = 4, 3, 16, 16, 19
    rng, m, feats, tokens, ctx, param = make(2, B, T, E, H, V, F32)
    lens = np.asarray([3, 1, 0, 2], np.int32)
    f = L.to_jl(feats)
    good = L.loss(ctx, param, f, vr.pad_with(tokens, lens, V - 1), lens=lens)
    bad = vr.pad_with(tokens, lens, 0)
    bad[0, 1] = V          # an active position
    with pytest.raises(lrcn_amd.LrcnError, match="token id"):
        L.loss(ctx, param, f, bad, lens=lens)
    assert L.loss(ctx, param, f, vr.pad_with(tokens, lens, 0), lens=lens) == good
    ctx.close()


def test_zero_length_rows_and_T0():
    B, E, H, V = 5, 24, 40, 31
    rng, m, feats, tokens, ctx, param = make(8, B, 3, E, H, V, F32)
    lens = np.asarray([0, 3, 0, 1, 0], np.int32)
    ref, ref_g = vr.loss(m, feats, tokens, lens, want_grad=True)
    g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens)
    assert abs(val - ref) <= 1e-5 * abs(ref)
    grads_close_f32(g, ref_g)
    empty = np.zeros((0, B), np.int32)
    ref0, ref0_g = orc.loss(m, feats, empty, want_grad=True)     # T = 0: every row is its eos term
    g0, val0 = L.lossgradient(ctx, param, L.to_jl(feats), empty, lens=[0] * B)
    assert abs(val0 - ref0) <= 1e-5 * abs(ref0)
    grads_close_f32(g0, ref0_g)
    all0 = L.loss(ctx, param, L.to_jl(feats), tokens, lens=[0] * B)   # T = 3, all rows empty: the same value
    assert abs(all0 - ref0) <= 1e-5 * abs(ref0)
    ctx.close()


def test_bad_arguments_return_einval_and_a_valid_call_still_works():
    B, T, E, H, V = 4, 3, 16, 16, 19
    rng, m, feats, tokens, ctx, param = make(2, B, T, E, H, V, F32)
    f, tok = L.to_jl(feats), torch.as_tensor(tokens).cuda()
    lib = _lib.lib()
    grads = [L.jl_empty(*t.shape) for t in param]
    out = C.c_double()

    def lens_p(v):
        a = np.asarray(v, np.int32)
        return a, a.ctypes.data_as(C.POINTER(C.c_int32))

    def call(lens, T_=T, B_=B, nt=10, drop=None, p=param, fe=f, g=grads):
        keep, lp = lens_p(lens) if lens is not None else (None, None)
        a = (ctx._h, L._p9(p) if p is not None else None, L._ptr(fe), C.c_void_p(tok.data_ptr()), lp, T_, B_, C.c_int64(nt), drop)
        return (lib.lrcn_loss_var(*a, C.byref(out)), lib.lrcn_loss_grad_var(*a, L._p9(g) if g is not None else None, C.byref(out)),
                lib.lrcn_train_step_var(ctx._h, L._p9(p) if p is not None else None, L._p9(grads), L._p9(grads), L._p9(grads), L._ptr(fe),
                                        C.c_void_p(tok.data_ptr()), lp, T_, B_, C.c_int64(nt), drop, 1, 1e-3, 0.9, 0.999, 1e-8, C.byref(out)))

    ok = [3, 1, 0, 2]
    EINVAL = (-1, -1, -1)
    assert call(None) == EINVAL and b"lens" in lib.lrcn_last_error(ctx._h)
    assert call([3, 1, 0, 4]) == EINVAL and call([3, -1, 0, 2]) == EINVAL
    assert call(ok, nt=0) == EINVAL and call(ok, nt=-5) == EINVAL
    # what lrcn_loss_grad rejects: shapes, dropout probability, null tensors
    assert call(ok, B_=0) == EINVAL and call(ok + [1], B_=B + 1) == EINVAL and call(ok, T_=-1) == EINVAL and call(ok, T_=T + 1) == EINVAL
    bad_drop = _lib.Dropout(1.0, 0, None, None)
    assert call(ok, drop=C.byref(bad_drop)) == EINVAL
    one_mask = _lib.Dropout(0.0, 0, f.data_ptr(), None)
    assert call(ok, drop=C.byref(one_mask)) == EINVAL
    assert call(ok, fe=None) == EINVAL
    keep, lp = lens_p(ok)
    assert lib.lrcn_loss_grad_var(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), lp, T, B, C.c_int64(10), None, _lib.P9(*([None] * 9)),
                                  C.byref(out)) == -1   # null gradient tensors
    ctx.sync()   # nothing was queued, nothing is pending
    ref = vr.loss(m, feats, tokens, ok)
    val = L.loss(ctx, param, f, tokens, lens=ok)
    assert abs(val - ref) <= 1e-5 * abs(ref)
    with pytest.raises(lrcn_amd.LrcnError):
        L.loss(ctx, param, f, tokens, lens=[1, 2, 3])   # the wrapper's own check: one length per row
    ctx.close()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_train_step_var_is_loss_grad_var_then_adam(dtype):
    B, T, E, H, V = 16, 6, 64, 64, 211
    rng, m, feats, tokens, ctx, _ = make(31, B, T, E, H, V, dtype, det=True)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    f = L.to_jl(feats)
    res = []
    for fused in (True, False):
        param = L.model_from_arrays(m.p)
        optim = L.initparams(param)
        grads = [L.jl_empty(*t.shape) for t in param]
        losses = []
        for step in range(3):
            if fused:
                losses.append(L.train_step(ctx, param, optim, grads, f, tokens, pdrop=0.4, seed=step, want_loss=True, lens=lens, norm_tokens=200))
            else:
                _, val = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=step, grads=grads, lens=lens, norm_tokens=200)
                L.update(ctx, param, grads, optim)
                losses.append(val)
        res.append((losses, host(param), host(optim.m), optim.t))
    (la, pa, ma, ta), (lb, pb, mb, tb) = res
    assert la == lb and ta == tb == 3
    for a, b in zip(pa + ma, pb + mb):
        assert np.array_equal(a, b)
    assert any(np.abs(a - L.from_jl(p0)).max() > 0 for a, p0 in zip(pa, L.model_from_arrays(m.p)) if a.size)
    ctx.close()


def scene_blocks(B=12):
    """Captions the image decides, of three lengths ("a dog runs", "the dog runs now", "a dog") -> padded (ids, tokens, lens) blocks, the
    feature table and the vocabulary size."""
    import json
    from lrcn_amd import captions as cap
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(48):
        n, v = nouns[img % 4], verbs[(img // 4) % 3]
        f = np.zeros(4096, np.float32)
        f[(img % 4) * 100:(img % 4) * 100 + 50] = 1.0
        f[1000 + ((img // 4) % 3) * 100:1000 + ((img // 4) % 3) * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns.append({"image_id": img, "caption": "A %s %s ." % (n, v)})
        anns.append({"image_id": img, "caption": "The %s %s now ." % (n, v)})
        if img % 3 == 0:
            anns.append({"image_id": img, "caption": "A %s ." % n})
    caps = cap.tokenize_coco(json.dumps({"annotations": anns}))
    vocab = cap.build_vocab([caps], threshold=1)
    return caps, vocab, cap.minibatch_varlen(caps, vocab, B), feats


def test_trainer_on_padded_blocks_lowers_the_loss_and_average_loss_is_the_token_weighted_mean():
    caps, vocab, blocks, feats = scene_blocks()
    assert sum(len(b[0]) for b in blocks) == len(caps) == 112 and any(len(set(b[2].tolist())) > 1 for b in blocks)
    E = H = 64
    V = len(vocab)
    ctx = L.Context(E, H, H, V, max_B=16, max_T=6, lstm_dtype=F32)
    ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    optim.lr = 0.01
    tr = dp.DataParallelTrainer(ctx, param, optim, 12, 1, 0, pdrop=0.0, seed=7)

    def feats_of(ids):
        return L.to_jl(np.stack([feats[i] for i in ids]).astype(np.float32))

    lines = []
    hist = trn.train(tr, [list(blocks), list(blocks)[:2]], 6, seed=3, feats_of=feats_of, log=lines.append, sync=ctx.sync)
    assert len(hist) == 6 and len(lines) == 6 and lines[0].startswith("(:epoch, 1, :loss, ")
    assert hist[-1][0] < 0.6 * hist[0][0], hist            # ln(V) ~ 2.6 at initialisation
    assert optim.t == 6 * len(blocks)
    # average_loss over the padded batches = the token-weighted mean of per-caption avg_loss_batch calls (equal-length entry point)
    got = trn.average_loss(tr, list(blocks), feats_of)
    total, count = 0.0, 0
    for ids, toks, lens in blocks:
        for b, i in enumerate(ids):
            n = int(lens[b])
            total += L.avg_loss_batch(ctx, param, feats_of([i]), toks[:n, b:b + 1]) * (n + 1)
            count += n + 1
    print("average_loss", got, "per-caption mean", total / count)
    assert abs(got - total / count) <= 1e-5 * abs(total / count)
    assert abs(got - hist[-1][0]) <= 1e-12
    tr.close()
    ctx.close()
