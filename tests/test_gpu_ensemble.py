"""GPU: ensemble beam search (lrcn_beam_ensemble_batch / lrcn_ensemble_mix_logits, include/lrcn_ensemble.h): the mix kernel on given logits
against the float64 definition (tests/ensemble_ref.py) in every load / store form; two small f32 models of different depth end to end
against the host searches over the wrapped oracle steps; constraints and groups through the ensemble; M = 1 is the constrained call bit
for bit; the parent hand-over on the bf16 cell-epilogue / table routes, on the plain route and between an f32 and a bf16 member;
repeatability, image independence, used contexts; argument errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as cr  # noqa: E402
import ensemble_ref as er  # noqa: E402
import nbest_ref as nb  # noqa: E402
from test_gpu_constrained import BANNED, MIN_LEN, NGRAM, assert_obeys  # noqa: E402  (that file's constraint set)
from test_gpu_nbest import compare, feats_of, small_model  # noqa: E402  (that file's comparison, tolerances and small model)

pytestmark = pytest.mark.gpu

N, NWORD, W = er.E2E_N, er.E2E_NWORD, er.E2E_W
EOS, BOS = lrcn_amd.EOS, lrcn_amd.BOS
_shared = {}


def teardown_module(module):
    for v in _shared.values():
        for ctx in v.get("ctxs", ()):
            ctx.close()
    _shared.clear()


def tokens(res):
    return [[e[0] for e in img] for img in res]


# ------------------------------------------------------------------------------------------------ 1. the mix kernel on given logits
def logit_ctx():
    if "logit" not in _shared:   # the entry does not depend on the context's sizes
        _shared["logit"] = {"ctxs": [L.Context(16, 16, 16, 20, max_B=8, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)]}
    return _shared["logit"]["ctxs"][0]


def device_view(a, ld, offset, dev):
    """a [R][V] as a device tensor view with row stride ld whose first element lies `offset` floats behind a 16-byte boundary"""
    R, V = a.shape
    buf = torch.full((R * ld + 4,), float("nan"), dtype=torch.float32, device=dev)   # nan between the rows: reading it would show
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + R * ld].view(R, ld)[:, :V]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 * (offset % 4) and v.stride(0) == ld
    return v


def member_layout(V, M):
    """(ld, offset) per member: member 0 on whole 16-byte rows (V = 1027: ld 1028), member 1 from a base that is not 16-byte aligned,
    member 2 on rows that are no multiple of 4 floats apart -- the scalar loads -- and unequal vector-form rows for the rest."""
    ld4 = (V + 3) // 4 * 4
    lay = [(ld4, 0), (ld4 + 4, 1), (ld4 + 7, 0)] + [(ld4 + 4 * m, 0) for m in range(3, 8)]
    return lay[:M]


@pytest.mark.parametrize("M", er.MIX_M)
@pytest.mark.parametrize("V", er.MIX_V)
def test_mix_kernel_against_the_definition(V, M):
    ctx = logit_ctx()
    dev = "cuda:%d" % ctx.device
    worst = 0.0
    for scale in er.MIX_SCALES:
        zs, w = er.mix_inputs(V, M, scale)
        wn = er.weights(w, M)
        # M = 1: the one member in the vector form at scale 1 and 40, in the scalar form (misaligned base) at scale 8
        lay = [(V + 5, 3)] if (M == 1 and scale == 8.0) else member_layout(V, M)
        views = [device_view(z, ld, off, dev) for z, (ld, off) in zip(zs, lay)]
        for mode in (er.PROB, er.LOGPROB):
            ref = er.mix(zs, wn, mode)
            x = L.ensemble_mix_logits(ctx, views, w, mode)
            assert x.shape == (er.MIX_R, V) and np.all(np.isfinite(x))
            e = er.mix_error(x, ref)
            worst = max(worst, e)
            assert e <= er.MIX_TOL, (V, M, scale, mode, e)
            assert L.ensemble_mix_logits(ctx, views, w, mode).tobytes() == x.tobytes()   # two identical calls: identical bits
            # the scalar stores: rows V + 1 floats apart from a base that is not 16-byte aligned; the same values, bit for bit
            out = device_view(np.zeros((er.MIX_R, V), np.float32), V + 1, 2, dev)
            y = L.ensemble_mix_logits(ctx, views, w, mode, out=out)
            assert y.tobytes() == x.tobytes()
        if scale == 1.0:   # numpy members (uploaded with ld = V) and uniform weights (NULL)
            x = L.ensemble_mix_logits(ctx, zs, None, er.PROB)
            e = er.mix_error(x, er.mix(zs, er.weights(None, M), er.PROB))
            worst = max(worst, e)
            assert e <= er.MIX_TOL, (V, M, "uniform", e)
    print("mix kernel V %d M %d: worst error %.3g of (1 + |v|)" % (V, M, worst))


def test_mix_kernel_leaves_the_row_padding_alone():
    ctx = logit_ctx()
    dev = "cuda:%d" % ctx.device
    V, M = 203, 3
    zs, w = er.mix_inputs(V, M, 8.0)
    views = [device_view(z, ld, off, dev) for z, (ld, off) in zip(zs, member_layout(V, M))]
    for ld, off in ((204, 0), (205, 1)):   # vector and scalar stores
        buf = torch.full((er.MIX_R * ld + 4,), -7.0, dtype=torch.float32, device=dev)
        out = buf[off:off + er.MIX_R * ld].view(er.MIX_R, ld)[:, :V]
        L.ensemble_mix_logits(ctx, views, w, er.PROB, out=out)
        full = buf.cpu().numpy()
        rows = full[off:off + er.MIX_R * ld].reshape(er.MIX_R, ld)
        assert np.all(rows[:, V:] == -7.0) and np.all(full[:off] == -7.0) and np.all(full[off + er.MIX_R * ld:] == -7.0)
        assert np.all(rows[:, :V] != -7.0)


# ------------------------------------------------------------------------------------------------ 2. two small f32 models end to end
def small():
    """member A: small_model(n_layers=2, seed=3), member B: a one-layer model of another seed; one context each, shared by the tests below"""
    if "small" not in _shared:
        ms = er.e2e_members(orc)
        assert np.array_equal(ms[0].p["Wout"], small_model(n_layers=2, seed=3).p["Wout"]) and ms[1].n_layers == 1
        ctxs = [L.Context(64, 64, 64, 203, max_B=N * 10, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=m.n_layers) for m in ms]
        feats = feats_of(N, 7)
        assert np.array_equal(feats, er.e2e_feats())
        _shared["small"] = {"ms": ms, "ctxs": ctxs, "params": [L.model_from_arrays(m.p) for m in ms], "feats": feats, "fj": L.to_jl(feats),
                            "refs": {}}
    return _shared["small"]


def small_reference(key, make):
    refs = small()["refs"]
    if key not in refs:
        refs[key] = make()
    return refs[key]


def host_step(S, mode, feats=None):
    feats = S["feats"] if feats is None else feats
    return er.EnsembleStep([nb.OracleStep(orc, m, feats) for m in S["ms"]], W, mode)


@pytest.mark.parametrize("mode", [er.PROB, er.LOGPROB])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_small_f32_against_host(K, alpha, mode):
    S = small()
    gpu = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, alpha, weights=W, mode=mode)
    for g in gpu:
        assert 1 <= len(g) <= K and all(g[q][2] >= g[q + 1][2] for q in range(len(g) - 1))
        for toks, lp, sc in g:
            assert toks[0] == BOS and (toks[-1] == EOS or len(toks) == NWORD + 2)
    ref = small_reference(("free", K, alpha, mode), lambda: cr.search(host_step(S, mode), N, K, NWORD, alpha))
    frac = compare(gpu, ref, label="ensemble %s K%d a%g" % (mode, K, alpha))
    print("ensemble f32 %s K%d alpha %g: %.1f %% of entries exact" % (mode, K, alpha, 100 * frac))
    assert frac >= 0.95, frac
    for ctx, param in zip(S["ctxs"], S["params"]):   # a driver that ignores a member cannot pass
        assert tokens(gpu) != tokens(L.beam_nbest_batch(ctx, param, S["fj"], K, NWORD, alpha))


# ------------------------------------------------------------------------------------------------ 3. constraints and groups
@pytest.mark.parametrize("mode", [er.PROB, er.LOGPROB])
def test_constraints_through_the_ensemble(mode):
    S = small()
    K, alpha = 3, 1.0
    gpu = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, alpha, W, mode, BANNED, MIN_LEN, NGRAM)
    free = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, alpha, W, mode)
    assert_obeys(gpu, BANNED, MIN_LEN, NGRAM)
    assert tokens(gpu) != tokens(free)   # the constraints bind
    ref = small_reference(("con", K, alpha, mode),
                          lambda: cr.search(host_step(S, mode), N, K, NWORD, alpha, allowed=cr.hook(BANNED, MIN_LEN, NGRAM)))
    frac = compare(gpu, ref, label="ensemble constrained %s" % mode)
    print("ensemble constrained %s: %.1f %% of entries exact" % (mode, 100 * frac))
    assert frac >= 0.95, frac


@pytest.mark.parametrize("mode", [er.PROB, er.LOGPROB])
def test_groups_through_the_ensemble(mode):
    S = small()
    K, G, lam, alpha = 6, 3, 0.5, 1.0
    gpu = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, alpha, W, mode, BANNED, MIN_LEN, NGRAM, groups=G, strength=lam)
    ref = cr.search_diverse(host_step(S, mode), N, K, G, lam, NWORD, alpha, allowed=cr.hook(BANNED, MIN_LEN, NGRAM))
    for img in gpu:
        assert len(img) == G
        assert_obeys(img, BANNED, MIN_LEN, NGRAM)
    frac = compare([g for img in gpu for g in img], [g for img in ref for g in img], label="ensemble diverse %s" % mode)
    print("ensemble diverse %s: %.1f %% of entries exact" % (mode, 100 * frac))
    assert frac >= 0.95, frac
    # groups without a constraint set: the empty ConstrainArgs
    gpu = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, alpha, W, mode, groups=G, strength=lam)
    ref = cr.search_diverse(host_step(S, mode), N, K, G, lam, NWORD, alpha)
    frac = compare([g for img in gpu for g in img], [g for img in ref for g in img], label="ensemble diverse free %s" % mode)
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 4. M = 1
def test_one_member_is_the_constrained_call_bit_for_bit():
    S = small()
    for ctx, param in zip(S["ctxs"], S["params"]):
        for cons in ({}, dict(banned=BANNED, min_len=MIN_LEN, no_repeat_ngram=NGRAM)):
            want = L.beam_constrained_batch(ctx, param, S["fj"], 5, NWORD, 0.5, **cons)
            assert L.beam_ensemble_batch([ctx], [param], S["fj"], 5, NWORD, 0.5, **cons) == want
            assert L.beam_ensemble_batch([ctx], [param], S["fj"], 5, NWORD, 0.5, weights=[2.5], mode=er.LOGPROB, **cons) == want
        want = L.beam_constrained_batch(ctx, param, S["fj"], 4, NWORD, 0.5, BANNED, MIN_LEN, NGRAM, groups=2, strength=0.8)
        assert L.beam_ensemble_batch([ctx], [param], S["fj"], 4, NWORD, 0.5, None, er.PROB, BANNED, MIN_LEN, NGRAM, groups=2, strength=0.8) == want


# ------------------------------------------------------------------------------------------------ 5. the parent hand-over on the bf16 routes
EB, VB, NB, KB, NWB, DEAD = 128, 1028, 52, 5, 8, 77   # 260 rows, bf16, H > 64, V % 4 == 0: the cell epilogue and the tables are on


def bf16():
    if "bf16" not in _shared:
        m = orc.init_weights(EB, EB, EB, VB, seed=5)
        m.p["Wout"][:] *= 8.0
        m.p["bout"][0, DEAD] = -1e4   # a word no row proposes: banning it cannot bind
        ctxs = [L.Context(EB, EB, EB, VB, max_B=NB * KB, max_T=2, lstm_dtype=dt) for dt in (lrcn_amd.LRCN_BF16, lrcn_amd.LRCN_BF16, lrcn_amd.LRCN_F32)]
        feats = feats_of(NB, 2)
        pick = np.linspace(0, NB - 1, 8).astype(int)
        _shared["bf16"] = {"m": m, "ctxs": ctxs, "param": L.model_from_arrays(m.p), "feats": feats, "fj": L.to_jl(feats), "pick": pick}
    return _shared["bf16"]


def bf16_host(B, members):
    """the host search over the picked images; members: per member whether its oracle step emulates bf16"""
    feats = B["feats"][B["pick"]]
    steps = [nb.OracleStep(orc, B["m"], feats, bf16=b) for b in members]
    step = steps[0] if len(steps) == 1 else er.EnsembleStep(steps, None, er.PROB)
    return nb.search(step, len(feats), KB, NWB, 1.0)


@pytest.mark.parametrize("epi", [True, False])
def test_one_bf16_model_in_two_contexts_is_the_single_context_call(monkeypatch, epi):
    B = bf16()
    if epi:
        monkeypatch.delenv("LRCN_DECODE_EPI", raising=False)   # the cell-epilogue and table routes: no follow_parents
    else:
        monkeypatch.setenv("LRCN_DECODE_EPI", "0")             # the plain route: follow_parents on every member
    c0, c1, _ = B["ctxs"]
    single = L.beam_constrained_batch(c0, B["param"], B["fj"], KB, NWB, 1.0, (DEAD,))
    ens = L.beam_ensemble_batch([c0, c1], [B["param"], B["param"]], B["fj"], KB, NWB, 1.0, None, er.PROB)
    frac = compare(ens, single, tol=1e-5, tie=1e-5, label="two bf16 contexts, epi %d" % epi)
    print("two bf16 contexts (epi %d): %.1f %% of entries exact" % (epi, 100 * frac))
    assert frac >= 0.95, frac
    if "host_bf16" not in B:
        B["host_bf16"] = bf16_host(B, [True])
    frac = compare([ens[i] for i in B["pick"]], B["host_bf16"], tol=2e-2, tie=2e-2, label="two bf16 contexts against the host")
    assert frac >= 0.9, frac


def test_an_f32_and_a_bf16_member(monkeypatch):
    monkeypatch.delenv("LRCN_DECODE_EPI", raising=False)
    B = bf16()
    c0, _, cf = B["ctxs"]
    ens = L.beam_ensemble_batch([cf, c0], [B["param"], B["param"]], B["fj"], KB, NWB, 1.0, None, er.PROB)   # the f32 member (plain route) leads
    frac = compare([ens[i] for i in B["pick"]], bf16_host(B, [False, True]), tol=2e-2, tie=2e-2, label="f32 + bf16 members")
    print("f32 + bf16 members: %.1f %% of entries exact" % (100 * frac))
    assert frac >= 0.9, frac
    swapped = L.beam_ensemble_batch([c0, cf], [B["param"], B["param"]], B["fj"], KB, NWB, 1.0, None, er.PROB)   # the bf16 member leads
    frac = compare(swapped, ens, tol=1e-5, tie=1e-5, label="f32 + bf16 members, swapped")
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 6. repeatability, independence, used contexts
def test_repeatable_independent_and_leaves_the_members_alone():
    S = small()
    K = 5
    own = [L.beam_nbest_batch(ctx, param, S["fj"], K, NWORD, 0.5) for ctx, param in zip(S["ctxs"], S["params"])]
    a = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, 0.5, W, er.PROB, BANNED, MIN_LEN, NGRAM)
    b = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, 0.5, W, er.PROB, BANNED, MIN_LEN, NGRAM)
    assert a == b
    sub = [2, 5, 6]
    c = L.beam_ensemble_batch(S["ctxs"], S["params"], L.to_jl(S["feats"][sub]), K, NWORD, 0.5, W, er.PROB, BANNED, MIN_LEN, NGRAM)
    assert c == [a[i] for i in sub]
    rev = L.beam_ensemble_batch(S["ctxs"][::-1], S["params"][::-1], S["fj"], K, NWORD, 0.5, W[::-1], er.LOGPROB)   # the other leader
    fwd = L.beam_ensemble_batch(S["ctxs"], S["params"], S["fj"], K, NWORD, 0.5, W, er.LOGPROB)
    assert compare(rev, fwd, label="leader swapped") >= 0.95
    for ctx, param, before in zip(S["ctxs"], S["params"], own):
        assert L.beam_nbest_batch(ctx, param, S["fj"], K, NWORD, 0.5) == before
    fresh = [L.Context(64, 64, 64, 203, max_B=N * 10, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=m.n_layers) for m in S["ms"]]
    d = L.beam_ensemble_batch(fresh, S["params"], S["fj"], K, NWORD, 0.5, W, er.PROB, BANNED, MIN_LEN, NGRAM)
    for ctx in fresh:
        ctx.close()
    assert d == a   # used contexts give a fresh pair's bits


# ------------------------------------------------------------------------------------------------ 7. argument errors
def test_argument_errors_return_einval():
    S = small()
    lib = _lib.lib()
    K, nword, n_img = 3, 6, 2
    fj = L.to_jl(feats_of(n_img, 1))
    out = (C.c_int32 * (n_img * K * (nword + 2)))()
    ln = (C.c_int * (n_img * K))()
    p9 = [L._p9(p) for p in S["params"]]
    other_v = L.Context(64, 64, 64, 207, max_B=N * 10, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    tight = L.Context(64, 64, 64, 203, max_B=n_img * K - 1, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    side = L.Context(64, 64, 64, 203, max_B=N * 10, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    stream = torch.cuda.Stream()
    side.use_stream(stream)
    good = [c._h.value for c in S["ctxs"]]

    def call(handles=good, params=p9, M=None, w=None, mode=0, N_=n_img, K_=K, G=0, lam=0.0, nword_=nword, alpha=0.0, cons=None, o=out, l=ln,
             feats=fj):
        M = len(handles) if M is None else M
        hs = (C.c_void_p * max(len(handles), 1))(*handles)
        ps = (C.c_void_p * max(len(params), 1))(*[C.addressof(p) if p is not None else None for p in params])
        wa = (C.c_float * len(w))(*w) if w is not None else None
        return lib.lrcn_beam_ensemble_batch(hs, ps, M, wa, mode, L._ptr(feats) if feats is not None else None, N_, K_, G, lam, nword_, alpha,
                                            C.byref(cons) if cons is not None else None, o, l, None, None)

    def einval(**kw):
        S["ctxs"][0].sync()
        assert call(**kw) == -1, kw   # LRCN_EINVAL
        assert lib.lrcn_last_error(S["ctxs"][0]._h)

    assert call() == 0
    assert call(w=[3.0, 1.0], mode=1) == 0
    einval(M=0)
    einval(handles=good * 5, params=p9 * 5, M=9)
    einval(handles=[good[0], None])
    einval(params=[p9[0], None])
    for w in ([0.0, 1.0], [-1.0, 1.0], [float("inf"), 1.0], [float("nan"), 1.0]):
        einval(w=w)
    einval(handles=good[:1], params=p9[:1], w=[0.0])   # M = 1: a weight, if given, must still be valid
    einval(mode=2)
    einval(mode=-1)
    einval(handles=[good[0], other_v._h.value])
    assert b"member 1" in lib.lrcn_last_error(S["ctxs"][0]._h)
    einval(handles=[good[0], side._h.value])
    assert b"member 1" in lib.lrcn_last_error(S["ctxs"][0]._h) and b"stream" in lib.lrcn_last_error(S["ctxs"][0]._h)
    einval(handles=[good[0], tight._h.value])
    assert b"member 1" in lib.lrcn_last_error(S["ctxs"][0]._h) and b"max_B" in lib.lrcn_last_error(S["ctxs"][0]._h)
    einval(handles=[good[0], good[0]], params=[p9[0], p9[0]])
    # everything lrcn_beam_constrained_batch rejects
    for kw in (dict(K_=0), dict(K_=33), dict(N_=0), dict(N_=N * 10), dict(nword_=0), dict(nword_=257), dict(alpha=-0.5), dict(alpha=float("nan")),
               dict(G=-1), dict(G=2), dict(K_=2, G=2, lam=-1.0), dict(o=None), dict(l=None), dict(feats=None)):
        einval(**kw)
    for ids, min_len, n in (([EOS], 0, 0), ([203], 0, 0), ([5, 9, 5], 0, 0), ([], nword + 1, 0), ([], -1, 0), ([], 0, -1),
                            (list(range(1, 203 - nword - K + 1)), 0, 0)):   # the last: V - nbanned - 1 - nword = K - 1
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        einval(cons=_lib.Constraints(arr, len(ids), min_len, n))
    # the kernel's own entry
    z = np.zeros((2, 20), np.float32)
    for bad in (dict(logits_list=[]), dict(logits_list=[z] * 9), dict(logits_list=[z, z], weights=[1.0, 0.0]), dict(logits_list=[z], mode="mean")):
        with pytest.raises(_lib.LrcnError):
            L.ensemble_mix_logits(S["ctxs"][0], **bad)
    dev = "cuda:%d" % S["ctxs"][0].device
    zt = torch.zeros((2, 20), dtype=torch.float32, device=dev)
    ptr = (C.c_void_p * 1)(zt.data_ptr())
    for ld, ld_out, R, V, md in ((19, 20, 2, 20, 0), (20, 19, 2, 20, 0), (20, 20, 0, 20, 0), (20, 20, 2, 0, 0), (20, 20, 2, 20, 2)):
        o = torch.zeros((2, 20), dtype=torch.float32, device=dev)
        assert lib.lrcn_ensemble_mix_logits(S["ctxs"][0]._h, ptr, (C.c_int64 * 1)(ld), 1, None, md, R, V, C.c_void_p(o.data_ptr()), ld_out) == -1
    assert lib.lrcn_ensemble_mix_logits(S["ctxs"][0]._h, ptr, (C.c_int64 * 1)(20), 1, None, 0, 2, 20, None, 20) == -1
    # nothing ran: the contexts are still usable and the good call still gives what it gave
    assert call() == 0
    first = list(out)
    assert call() == 0 and list(out) == first
    for c in (other_v, tight, side):
        c.close()
