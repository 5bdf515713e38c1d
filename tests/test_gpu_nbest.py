"""GPU: the n-best beam search (lrcn_beam_nbest_batch, include/lrcn_nbest.h) against the host restatement driven by the CPU oracle
(tests/nbest_ref.py) on small f32 models and the bf16 production shape, on both routes of its log-probability top-K (the logits GEMM's
records merge and the rows kernel on f32 logits); K = 1 against lrcn_beam_search_batch; logp against lrcn_score_pairs and a teacher-forced
oracle sum in the regime where the reference beam's probability product underflows; repeatability, image independence and argument errors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nbest_ref as nb  # noqa: E402

pytestmark = pytest.mark.gpu

E = H = 1000
V = 10640      # the production decode shape: 1024 images x 5 beams = 5120 rows
NP, KP, NWORD = 1024, 5, 8


def decisive_model(seed=4):
    """As in test_gpu_decode_epilogue.py: random weights scaled until the word distributions are peaky (no near-ties)."""
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed)
    for n in ("W1", "W2", "Wout"):
        m.p[n] *= 2.0
    m.p["Wout"][:] *= 8.0
    m.p["bout"][:] = (rng.standard_normal((1, V)) * 2.0).astype(np.float32)
    m.p["b1"][:] += (rng.standard_normal(m.p["b1"].shape) * 0.5).astype(np.float32)
    return m


def small_model(n_layers=2, seed=3, Vs=203, Es=64, spread=16.0):
    m = orc.init_weights(Es, Es, Es, Vs, seed=seed, n_layers=n_layers)
    m.p["Wout"][:] *= spread   # spread in the word distributions: fewer near-ties among the n best, still far from peaky
    return m


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


_production = {}


def production():
    """One bf16 context + decisive model at the production shape, shared by the tests of this file (the context holds ~1 GB of tables)."""
    if not _production:
        m = decisive_model()
        ctx = L.Context(E, H, H, V, max_B=NP * KP, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        _production.update(m=m, ctx=ctx, param=L.model_from_arrays(m.p), feats=feats_of(NP, 11))
    return _production


def teardown_module(module):
    if _production:
        _production["ctx"].close()
        _production.clear()


def host(m, feats, K, nword, alpha, bf16=False):
    return nb.search(nb.OracleStep(orc, m, feats, bf16=bf16), len(feats), K, nword, alpha)


def compare(gpu, ref, tol=1e-5, tie=1e-5, label=""):
    """Entry by entry, best first: identical tokens (then logp / score within tol (1 + |v|)), or a logged near-tie -- the host's scores of
    the two orderings (its own score of the GPU's entry if it has one, else the GPU's score) differ by at most tie (1 + |s|).
    Returns the fraction of exact entries."""
    entries = exact = 0
    for n, (g, r) in enumerate(zip(gpu, ref)):
        assert len(g) == len(r), (label, n, len(g), len(r))
        host_score = {tuple(e[0]): float(e[2]) for e in r}
        for q, ((gt, glp, gsc), (rt, rlp, rsc)) in enumerate(zip(g, r)):
            entries += 1
            if gt == rt:
                exact += 1
                assert abs(glp - float(rlp)) <= tol * (1 + abs(float(rlp))), (label, n, q, glp, rlp)
                assert abs(gsc - float(rsc)) <= tol * (1 + abs(float(rsc))), (label, n, q, gsc, rsc)
            else:
                other = host_score.get(tuple(gt), gsc)
                gap = abs(other - float(rsc))
                print("near-tie %s image %d entry %d: host gap %.3g (gpu %r, host %r)" % (label, n, q, gap, gsc, float(rsc)))
                assert gap <= tie * (1 + abs(float(rsc))), (label, n, q, gt, rt, gsc, float(rsc), other)
    return exact / max(entries, 1)


# ------------------------------------------------------------------------------------------------ 1. small f32 models against the host
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("K", [1, 3, 10, 32])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_small_f32_against_host(n_layers, K, alpha):
    m = small_model(n_layers=n_layers)
    N, nword = (4 if K == 32 else 8), 12
    ctx = L.Context(64, 64, 64, 203, max_B=N * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)
    param = L.model_from_arrays(m.p)
    feats = feats_of(N, 7)
    gpu = L.beam_nbest_batch(ctx, param, L.to_jl(feats), K, nword, alpha)
    ctx.close()
    ref = host(m, feats, K, nword, alpha)
    for g in gpu:
        assert 1 <= len(g) <= K
        assert all(g[q][2] >= g[q + 1][2] for q in range(len(g) - 1))
        for toks, lp, sc in g:
            assert toks[0] == lrcn_amd.BOS and (toks[-1] == lrcn_amd.EOS or len(toks) == nword + 2)
    frac = compare(gpu, ref, label="f32 L%d K%d a%g" % (n_layers, K, alpha))
    print("f32 L%d K%d alpha %g: %.1f %% of entries exact" % (n_layers, K, alpha, 100 * frac))
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 2. K = 1, alpha 0 == the reference beam at width 1
def test_k1_equals_beam_search_width_1_f32():
    m = small_model()
    N = 12
    ctx = L.Context(64, 64, 64, 203, max_B=N, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 1))
    beam = L.beam_search_batch(ctx, param, fj, 1, 12)
    nbest = L.beam_nbest_batch(ctx, param, fj, 1, 12, 0.0)
    assert [t for t, _ in beam] == [img[0][0] for img in nbest]
    ctx.close()


def test_k1_equals_beam_search_width_1_bf16_production():
    P = production()
    N = NP * KP
    fj = L.to_jl(feats_of(N, 2))
    beam = L.beam_search_batch(P["ctx"], P["param"], fj, 1, NWORD)
    nbest = L.beam_nbest_batch(P["ctx"], P["param"], fj, 1, NWORD, 0.0)
    assert [t for t, _ in beam] == [img[0][0] for img in nbest]


# ------------------------------------------------------------------------------------------------ 3. production shape: fused route vs rows kernel, and the host
def test_production_bf16_routes_agree_and_match_host(monkeypatch):
    P = production()
    fj = L.to_jl(P["feats"])
    monkeypatch.setenv("LRCN_DECODE_SMAX", "1")
    fused = L.beam_nbest_batch(P["ctx"], P["param"], fj, KP, NWORD, 0.0)
    monkeypatch.setenv("LRCN_DECODE_SMAX", "0")
    rows = L.beam_nbest_batch(P["ctx"], P["param"], fj, KP, NWORD, 0.0)
    assert [[e[0] for e in img] for img in fused] == [[e[0] for e in img] for img in rows]
    for a, b in zip(fused, rows):
        for (_, la, _), (_, lb, _) in zip(a, b):
            assert abs(la - lb) <= 1e-5 * (1 + abs(lb)), (la, lb)
    pick = np.linspace(0, NP - 1, 16).astype(int)
    ref = host(P["m"], P["feats"][pick], KP, NWORD, 0.0, bf16=True)
    frac = compare([fused[i] for i in pick], ref, tol=2e-2, tie=2e-2, label="bf16 production")
    assert frac >= 0.9, frac


# ------------------------------------------------------------------------------------------------ 4. K = 10 at the production vocabulary (rows kernel)
def test_k10_production_vocabulary_against_host():
    P = production()
    N, K = 8, 10
    feats = P["feats"][:N]
    gpu = L.beam_nbest_batch(P["ctx"], P["param"], L.to_jl(feats), K, NWORD, 1.0)
    ref = host(P["m"], feats, K, NWORD, 1.0, bf16=True)
    frac = compare(gpu, ref, tol=2e-2, tie=2e-2, label="K10 V10640")
    assert frac >= 0.9, frac


# ------------------------------------------------------------------------------------------------ 5. logp == lrcn_score_pairs of the entry
def test_logp_equals_caption_score():
    m = small_model()
    m.p["bout"][0, lrcn_amd.EOS] += 6.0   # captions that end in eos
    N, K, nword = 8, 3, 12
    ctx = L.Context(64, 64, 64, 203, max_B=N * K * 4, max_T=28, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 5))
    res = L.beam_nbest_batch(ctx, param, fj, K, nword, 1.0)
    caps, img, lps, scs = [], [], [], []
    for n, entries in enumerate(res):
        for toks, lp, sc in entries:
            words = toks[1:-1]
            if toks[-1] == lrcn_amd.EOS and 1 <= len(words) <= 27:
                caps.append(words); img.append(n); lps.append(lp); scs.append(sc)
    assert len(caps) >= N
    s = L.score_pairs(ctx, param, fj, caps, img, list(range(len(caps))))
    for c, sv, lp, sc in zip(caps, s, lps, scs):
        assert abs(lp - sv) <= 1e-4 * (1 + abs(sv)), (c, lp, sv)
        assert abs(sc - sv / (len(c) + 1)) <= 1e-4 * (1 + abs(sv)), (c, sc, sv)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the underflow regime of the reference beam
def test_flat_model_logp_is_finite_and_teacher_forced():
    m = small_model(spread=4.0)
    m.p["Wout"][:] *= 1e-3
    m.p["bout"][0, lrcn_amd.EOS] = -3.0   # captions run to the length limit
    N, K, nword = 6, 4, 30
    ctx = L.Context(64, 64, 64, 203, max_B=N * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    feats = feats_of(N, 9)
    fj = L.to_jl(feats)
    beam = L.beam_search_batch(ctx, param, fj, K, nword)
    assert any(p == 0.0 for _, p in beam)   # the product of float32 probabilities underflows
    res = L.beam_nbest_batch(ctx, param, fj, K, nword, 0.0)
    ctx.close()
    rows = [(n, toks, lp) for n, entries in enumerate(res) for toks, lp, _ in entries]
    assert len(rows) == N * K
    T = max(max(len(t) for _, t, _ in rows) - 2, 1)
    tok = np.zeros((T, len(rows)), np.int32)
    for b, (_, t, _) in enumerate(rows):
        for q in range(len(t) - 2):
            tok[q, b] = t[q + 1]
    z = orc.forward_logits(m, np.stack([feats[n] for n, _, _ in rows]), tok)
    for b, (_, t, lp) in enumerate(rows):
        assert np.isfinite(lp)
        ref = sum(float(nb.log_softmax(z[q, b])[t[q + 1]]) for q in range(len(t) - 1))
        assert abs(lp - ref) <= 1e-4 * (1 + abs(ref)), (b, lp, ref)


# ------------------------------------------------------------------------------------------------ 7. repeatability and independence
def test_repeatable_independent_and_leaves_the_beam_alone():
    m = small_model()
    N, K = 8, 5
    ctx = L.Context(64, 64, 64, 203, max_B=N * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    feats = feats_of(N, 3)
    fj = L.to_jl(feats)
    beam0 = L.beam_search_batch(ctx, param, fj, K, 12)
    a = L.beam_nbest_batch(ctx, param, fj, K, 12, 0.5)
    b = L.beam_nbest_batch(ctx, param, fj, K, 12, 0.5)
    assert a == b
    sub = [2, 5, 6]
    c = L.beam_nbest_batch(ctx, param, L.to_jl(feats[sub]), K, 12, 0.5)
    assert c == [a[i] for i in sub]
    beam1 = L.beam_search_batch(ctx, param, fj, K, 12)
    assert beam0 == beam1
    ctx.close()


def test_repeatable_production_fused():
    P = production()
    fj = L.to_jl(P["feats"])
    a = L.beam_nbest_batch(P["ctx"], P["param"], fj, KP, NWORD, 1.0)
    b = L.beam_nbest_batch(P["ctx"], P["param"], fj, KP, NWORD, 1.0)
    assert a == b


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_argument_errors_return_einval():
    m = small_model()
    N = 4
    ctx = L.Context(64, 64, 64, 203, max_B=8, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 1))
    lib = _lib.lib()
    out = (C.c_int32 * (N * 8 * 300))()
    n = (C.c_int * (N * 8))()
    lp = (C.c_float * (N * 8))()
    sc = (C.c_float * (N * 8))()

    def call(N_, K, nword, alpha, o=out, ln=n, feats=fj):
        return lib.lrcn_beam_nbest_batch(ctx._h, L._p9(param), L._ptr(feats) if feats is not None else None, N_, K, nword, alpha, o, ln, lp, sc)

    assert call(N, 2, 4, 0.0) == 0
    assert lib.lrcn_beam_nbest_batch(ctx._h, L._p9(param), L._ptr(fj), N, 2, 4, 1.0, out, n, None, None) == 0
    bad = [(N, 0, 4, 0.0), (N, 3, 4, 0.0), (N, 33, 4, 0.0), (0, 1, 4, 0.0),          # K < 1, N*K > max_B, K > 32, N < 1
           (N, 1, 4, -0.5), (N, 1, 4, float("nan")), (N, 1, 4, float("inf")),
           (N, 1, 0, 0.0), (N, 1, 257, 0.0)]
    for args in bad:
        assert call(*args) == -1, args   # LRCN_EINVAL
        assert lib.lrcn_last_error(ctx._h)
    assert call(N, 1, 4, 0.0, o=None) == -1
    assert call(N, 1, 4, 0.0, ln=None) == -1
    assert call(N, 1, 4, 0.0, feats=None) == -1
    ctx.close()
    tiny = L.Context(16, 16, 16, 20, max_B=64, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    mt = orc.init_weights(16, 16, 16, 20, seed=1)
    pt = L.model_from_arrays(mt.p)
    f1 = L.to_jl(feats_of(1, 1))
    assert lib.lrcn_beam_nbest_batch(tiny._h, L._p9(pt), L._ptr(f1), 1, 21, 4, 0.0, out, n, lp, sc) == -1   # K > V
    assert lib.lrcn_beam_nbest_batch(tiny._h, L._p9(pt), L._ptr(f1), 1, 20, 4, 0.0, out, n, lp, sc) == 0
    tiny.close()
