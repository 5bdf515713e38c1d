"""GPU: the weighted caption loss, gradient and training step (include/lrcn_weighted.h) against tests/weighted_ref.py -- the per-caption
sums of the equal-length CPU oracle, each times its row's weight.

Tolerances are the ones tests/test_gpu_varlen.py states and uses: f32 loss 1e-5 relative, f32 gradients rtol 1e-3 + atol 1e-5; bf16 the
two bounds of tests/parity_util.py.  With every weight 1.0f a deterministic context must return the bits of lrcn_loss_grad_var: the
kernel's scale * 1.0f is the same float and no further row is masked."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib, dp
from lrcn_amd import lrcn as L
from oracle import oracle as orc
from parity_util import assert_bf16_matches_emulation, assert_bf16_near_f32_oracle

import varlen_ref as vr
import weighted_ref as wr

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
NAMES = ("lrcn_loss_w", "lrcn_loss_grad_w", "lrcn_train_step_w")
ALWAYS = 1e-3   # tests/test_gpu_clip.py's: far below any gradient norm met here, every step clips


def make(seed, B, T, E, H, V, dtype, n_layers=2, det=False):
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


def mixed_case(rng, B, T):
    """Lengths with a row of length T and one of length 0; normal weights with at least one negative and one exactly 0."""
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    w = rng.standard_normal(B).astype(np.float32)
    w[0], w[1], w[2], w[3] = -abs(w[0]) - 0.25, abs(w[1]) + 0.25, 0.0, abs(w[3]) + 0.25
    return lens, w


def test_the_three_exports_exist():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
    assert set(_lib.WEIGHTED_SIGNATURES) == set(NAMES)
    assert lib.lrcn_abi_version() == 5


@pytest.mark.parametrize("pdrop", [0.0, 0.4])
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_weights_of_one_are_bit_identical_to_loss_grad_var(dtype, n_layers, pdrop):
    B, T, E, H, V = 24, 6, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(11, B, T, E, H, V, dtype, n_layers, det=True)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    one = np.ones(B, np.float32)
    f = L.to_jl(feats)
    for nt in (None, 4 * vr.norm_tokens_of(lens)):
        ga, la = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=nt)
        ga = host(ga)
        lf = L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=nt)
        gb, lb = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=nt, row_weights=one)
        gb = host(gb)
        assert L.last_loss(ctx) == lb
        lg = L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, norm_tokens=nt, row_weights=one)
        assert la == lb and lf == lg and L.last_loss(ctx) == lg
        for k, (a, b) in enumerate(zip(ga, gb)):
            assert np.array_equal(a, b), "gradient %d differs from lrcn_loss_grad_var's" % k
        assert any(np.abs(a).max() > 0 for a in ga)
    ctx.close()


@pytest.mark.parametrize("n_layers,masks,B,T,E,H,V", [(2, True, 13, 7, 52, 36, 97), (1, False, 11, 6, 40, 48, 203), (2, False, 6, 3, 16, 16, 16400)])
def test_mixed_signs_f32_vs_reference(n_layers, masks, B, T, E, H, V):
    # V = 97, 203: odd widths (the scalar tail of the register-resident kernel); V = 16400: the generic kernel above its 16384 columns
    rng, m, feats, tokens, ctx, param = make(B + T, B, T, E, H, V, F32, n_layers)
    lens, w = mixed_case(rng, B, T)
    assert (w < 0).any() and (w == 0).any() and (lens == 0).any() and (lens == T).any()
    kw = {}
    if masks:
        kw["mask1"] = ((rng.random((T + 1, B, E)) > 0.4) / 0.6).astype(np.float32)
        kw["mask2"] = ((rng.random((T + 1, B, H)) > 0.4) / 0.6).astype(np.float32)
    for nt in (None, 3 * vr.norm_tokens_of(lens)):   # the batch's own count, and a "global" one
        ref, ref_g = wr.loss(m, feats, tokens, lens, w, nt, want_grad=True, **kw)
        for _ in range(2):   # twice: scratch carries the first pass's values
            g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=nt, row_weights=w, **kw)
            print("f32 weighted: loss", val, "ref", ref, "rel", abs(val - ref) / abs(ref))
            assert abs(val - ref) <= 1e-5 * abs(ref)
            grads_close_f32(g, ref_g)
        only = L.loss(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=nt, row_weights=w, **kw)
        assert abs(only - ref) <= 1e-5 * abs(ref)
    ctx.close()


@pytest.mark.parametrize("B", [256, 48])
def test_power_of_two_weights_bf16_vs_emulating_oracle(B):
    # 256 rows: GEMM + cell kernel per recurrence step; 48 rows: the fused step kernels.  Weights +-0.5, +-1, +-2 and lengths with integer
    # shares: the oracle's row b rounds d(logits) at the library's scale |w[b]| / norm_tokens (tests/weighted_ref.py)
    T, E, H, V = 5, 64, 64, 157
    rng, m, feats, tokens, ctx, param = make(B, B, T, E, H, V, BF16)
    lens, w, nt = wr.bf16_case(B, np.random.default_rng(B))
    assert lens.max() <= T
    ref, ref_g = wr.emulated_reference(m, feats, tokens, lens, w, nt)
    g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=nt, row_weights=w)
    print("bf16 weighted B=%d: loss" % B, val, "emulated", ref, "f32", ref_g.f32[0])
    assert_bf16_matches_emulation(val, g, ref, ref_g, "weighted bf16 B=%d" % B)
    ctx.close()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_a_zero_weight_row_is_not_read_past_the_loss_kernel(dtype):
    B, T, E, H, V = 33, 8, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(21, B, T, E, H, V, dtype, det=True)
    lens, w = mixed_case(rng, B, T)
    zero = [2, 5, 6, 17, 32]
    w[zero] = 0.0
    lens[5], lens[17] = T, 3            # zero-weight rows with active steps
    other = tokens.copy()
    other[:, zero] = 3 + (other[:, zero] - 3 + 1 + rng.integers(0, V - 4, size=(T, len(zero)))) % (V - 3)   # other valid ids, every one changed
    assert (other[:, zero] != tokens[:, zero]).all() and (other >= 3).all() and (other < V).all()
    f = L.to_jl(feats)
    ga, la = L.lossgradient(ctx, param, f, tokens, lens=lens, row_weights=w, pdrop=0.3, seed=4)
    ga = host(ga)
    gb, lb = L.lossgradient(ctx, param, f, other, lens=lens, row_weights=w, pdrop=0.3, seed=4)
    gb = host(gb)
    assert la == lb
    for k, (a, b) in enumerate(zip(ga, gb)):
        assert np.array_equal(a, b), "gradient %d depends on a zero-weight row's tokens" % k
    # against the reference with those rows omitted (norm_tokens kept), without dropout
    keep = [b for b in range(B) if b not in zero]
    nt = vr.norm_tokens_of(lens)
    f32_loss, f32_g = wr.loss(m, feats[keep], tokens[:, keep], lens[keep], w[keep], nt, want_grad=True)
    for toks in (tokens, other):
        g, val = L.lossgradient(ctx, param, f, toks, lens=lens, row_weights=w)
        if dtype == F32:
            assert abs(val - f32_loss) <= 1e-5 * abs(f32_loss)
            grads_close_f32(g, f32_g)
        else:
            assert_bf16_near_f32_oracle(val, g, f32_loss, f32_g, "weighted, zero-weight rows")
    ctx.close()


@pytest.mark.parametrize("gclip", [0.0, ALWAYS, 1e30])
def test_train_step_w_is_loss_grad_w_then_update(gclip):
    B, T, E, H, V = 16, 6, 64, 64, 211
    rng, m, feats, tokens, ctx, _ = make(31, B, T, E, H, V, BF16, det=True)
    lens, w = mixed_case(rng, B, T)
    f = L.to_jl(feats)
    res = []
    for fused in (True, False):
        param = L.model_from_arrays(m.p)
        optim = L.initparams(param)
        grads = [L.jl_empty(*t.shape) for t in param]
        losses, norms = [], []
        for step in range(3):
            if fused:
                losses.append(L.train_step(ctx, param, optim, grads, f, tokens, pdrop=0.4, seed=step, want_loss=True, lens=lens, norm_tokens=200,
                                           row_weights=w, gclip=gclip))
            else:
                _, val = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=step, grads=grads, lens=lens, norm_tokens=200, row_weights=w)
                if gclip > 0:
                    L.grad_sumsq(ctx, grads)
                    L.clip_set(ctx, gclip)
                L.update(ctx, param, grads, optim, clipped=gclip > 0)
                losses.append(val)
            if gclip > 0:
                st = L.clip_stats(ctx)
                norms.append((st["last_norm"], st["last_scale"], st["last_skipped"]))
        res.append((losses, host(param), host(optim.m), host(optim.v), optim.t, norms))
    (la, pa, ma, va, ta, na), (lb, pb, mb, vb, tb, nb) = res
    print("gclip", gclip, "losses", la, "norms", na)
    assert la == lb and ta == tb == 3 and na == nb
    for a, b in zip(pa + ma + va, pb + mb + vb):
        assert np.array_equal(a, b)
    assert any(np.abs(a - L.from_jl(p0)).max() > 0 for a, p0 in zip(pa, L.model_from_arrays(m.p)) if a.size)
    if gclip == ALWAYS:
        assert all(s < 1.0 for _, s, _ in na), na
    elif gclip > 0:
        assert all(s == 1.0 for _, s, _ in na)
    ctx.close()


def test_bad_arguments_return_einval_and_a_valid_call_still_works():
    B, T, E, H, V = 4, 3, 16, 16, 19
    rng, m, feats, tokens, ctx, param = make(2, B, T, E, H, V, F32)
    f, tok = L.to_jl(feats), torch.as_tensor(tokens).cuda()
    lib = _lib.lib()
    grads = [L.jl_empty(*t.shape) for t in param]
    out = C.c_double()

    def arr(v, dt, ct):
        a = np.asarray(v, dt)
        return a, a.ctypes.data_as(C.POINTER(ct))

    def call(lens, w, T_=T, B_=B, nt=10, drop=None, p=param, fe=f, g=grads):
        kl, lp = arr(lens, np.int32, C.c_int32) if lens is not None else (None, None)
        kw, wp = arr(w, np.float32, C.c_float) if w is not None else (None, None)
        a = (ctx._h, L._p9(p) if p is not None else None, L._ptr(fe), C.c_void_p(tok.data_ptr()), lp, wp, T_, B_, C.c_int64(nt), drop)
        return (lib.lrcn_loss_w(*a, C.byref(out)), lib.lrcn_loss_grad_w(*a, L._p9(g) if g is not None else None, C.byref(out)),
                lib.lrcn_train_step_w(ctx._h, L._p9(p) if p is not None else None, L._p9(grads), L._p9(grads), L._p9(grads), L._ptr(fe),
                                      C.c_void_p(tok.data_ptr()), lp, wp, T_, B_, C.c_int64(nt), drop, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, C.byref(out)))

    ok, okw = [3, 1, 0, 2], [1.0, -0.5, 0.0, 2.0]
    EINVAL = (-1, -1, -1)
    assert call(ok, None) == EINVAL and b"row_w" in lib.lrcn_last_error(ctx._h)
    assert call(ok, [1.0, float("nan"), 0.0, 2.0]) == EINVAL and b"finite" in lib.lrcn_last_error(ctx._h)
    assert call(ok, [1.0, float("inf"), 0.0, 2.0]) == EINVAL and call(ok, [1.0, -float("inf"), 0.0, 2.0]) == EINVAL
    assert call(None, okw) == EINVAL and b"lens" in lib.lrcn_last_error(ctx._h)
    # what lrcn_loss_grad_var rejects: lengths, the normaliser, shapes, dropout probability, one mask of two, null tensors
    assert call([3, 1, 0, 4], okw) == EINVAL and call([3, -1, 0, 2], okw) == EINVAL
    assert call(ok, okw, nt=0) == EINVAL and call(ok, okw, nt=-5) == EINVAL
    assert call(ok, okw, B_=0) == EINVAL and call(ok + [1], okw + [1.0], B_=B + 1) == EINVAL and call(ok, okw, T_=-1) == EINVAL
    assert call(ok, okw, T_=T + 1) == EINVAL
    bad_drop = _lib.Dropout(1.0, 0, None, None)
    assert call(ok, okw, drop=C.byref(bad_drop)) == EINVAL
    one_mask = _lib.Dropout(0.0, 0, f.data_ptr(), None)
    assert call(ok, okw, drop=C.byref(one_mask)) == EINVAL
    assert call(ok, okw, fe=None) == EINVAL
    (kl, lp), (kw, wp) = arr(ok, np.int32, C.c_int32), arr(okw, np.float32, C.c_float)
    assert lib.lrcn_loss_grad_w(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), lp, wp, T, B, C.c_int64(10), None, _lib.P9(*([None] * 9)),
                                C.byref(out)) == -1   # null gradient tensors
    assert lib.lrcn_train_step_w(ctx._h, L._p9(param), L._p9(grads), L._p9(grads), L._p9(grads), L._ptr(f), C.c_void_p(tok.data_ptr()), lp, wp, T, B,
                                 C.c_int64(10), None, 1, 1e-3, 0.9, 0.999, 1e-8, float("nan"), C.byref(out)) == -1   # a NaN max_norm
    ctx.sync()   # nothing was queued, nothing is pending
    ref = wr.loss(m, feats, tokens, ok, okw)
    val = L.loss(ctx, param, f, tokens, lens=ok, row_weights=okw)
    assert abs(val - ref) <= 1e-5 * abs(ref)
    with pytest.raises(lrcn_amd.LrcnError):
        L.loss(ctx, param, f, tokens, lens=ok, row_weights=[1.0, 2.0, 3.0])   # the wrapper's own checks: one weight per row,
    with pytest.raises(lrcn_amd.LrcnError):
        L.lossgradient(ctx, param, f, tokens, row_weights=okw)               # and weights need lens
    optim = L.initparams(param)
    with pytest.raises(lrcn_amd.LrcnError):
        L.train_step(ctx, param, optim, grads, f, tokens, row_weights=okw)
    assert optim.t == 0
    ctx.close()


@pytest.fixture
def one_rank_nccl():
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def test_trainer_step_with_row_weights_pipeline_and_gclip_equal_the_plain_path(monkeypatch, one_rank_nccl):
    for k in ("LRCN_DP_FORCE_PIPELINE", "LRCN_DP_SPARSE_EMBED", "LRCN_DP_SHARD_ADAM", "LRCN_DP_GROUP_ADAM", "LRCN_DP_BUCKETS", "LRCN_DP_BACKEND",
              "LRCN_FUSED_UPDATE"):
        monkeypatch.delenv(k, raising=False)
    B, T, E, H, V = 16, 6, 64, 64, 211
    rng = np.random.default_rng(5)
    steps = []
    for _ in range(3):
        lens, w = mixed_case(rng, B, T)
        steps.append(((rng.standard_normal((B, 4096)) * 0.02).astype(np.float32), rng.integers(3, V, size=(T, B)).astype(np.int32), lens, w))

    def run(pipeline, gclip):
        monkeypatch.setenv("LRCN_DP_FORCE_PIPELINE", "1" if pipeline else "0")
        ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=BF16)
        try:
            ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
            param = L.initweights(ctx, seed=42)
            tr = dp.DataParallelTrainer(ctx, param, L.initparams(param), B, 1, 0, pdrop=0.4, seed=7, group=one_rank_nccl if pipeline else None,
                                        backend="torch", gclip=gclip)
            assert tr._group_pipeline() == pipeline
            losses = []
            for feats, toks, lens, w in steps:
                tr.step(None, toks, feats=L.to_jl(feats), lens=lens, row_weights=w)
                losses.append(tr.loss_value())
            out = (host(param), losses, tr.clip_stats() if gclip > 0 else None)
            tr.close()
            return out
        finally:
            ctx.close()

    for gclip in (0.0, ALWAYS):
        (pa, la, sa), (pb, lb, sb) = run(False, gclip), run(True, gclip)
        print("gclip", gclip, "losses", la, "stats", sa)
        assert la == lb
        for k, (a, b) in enumerate(zip(pa, pb)):
            assert np.array_equal(a, b), "parameter %d: pipeline differs from the plain path" % k
        if gclip > 0:
            assert sa["steps"] == sb["steps"] == 3 and sa["clipped"] == sb["clipped"] == 3 and sa["last_norm"] == sb["last_norm"]
