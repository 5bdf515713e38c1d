"""GPU: diverse beam search (lrcn_beam_diverse_batch, include/lrcn_diverse.h): one group is lrcn_beam_nbest_batch bit for bit (small f32
models and the bf16 production route); groups against the host restatement driven by the CPU oracle (tests/diverse_ref.py) on the cases of
tests/diverse_cases.py; strength 0 repeats group 0; logp is the model's log-likelihood of the caption (lrcn_score_pairs), not the penalised
value; a large strength keeps the groups' words apart; repeatability, image independence, no trace left for the other beams; argument
errors."""
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
import diverse_ref as dv  # noqa: E402
import diverse_cases as dc  # noqa: E402
from test_gpu_nbest import compare, decisive_model  # noqa: E402  (that file's comparison and tolerances, and its production model)

pytestmark = pytest.mark.gpu

NWORD = dc.NWORD
_small = {}        # n_layers -> (context, device parameters), max_B = 128 rows: every small case of this file
_production = {}


def small(n_layers=2):
    if n_layers not in _small:
        ctx = L.Context(dc.ES, dc.ES, dc.ES, dc.VS, max_B=128, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)
        _small[n_layers] = (ctx, L.model_from_arrays(dc.small_model(n_layers=n_layers).p))
    return _small[n_layers]


def production():
    """One bf16 context + decisive model at the production sizes (E = H = 1000, V = 10640), 5120 rows"""
    if not _production:
        m = decisive_model()
        ctx = L.Context(1000, 1000, 1000, 10640, max_B=5120, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        _production.update(ctx=ctx, param=L.model_from_arrays(m.p))
    return _production


def teardown_module(module):
    for ctx, _ in _small.values():
        ctx.close()
    _small.clear()
    if _production:
        _production["ctx"].close()
        _production.clear()


def groups_of(res):
    return [grp for img in res for grp in img]


# ------------------------------------------------------------------------------------------------ 1. one group == the n-best beam, bit for bit
@pytest.mark.parametrize("lam", [0.0, 0.7])
@pytest.mark.parametrize("K", [3, 10, 32])
def test_one_group_is_nbest_bit_for_bit_f32(K, lam):
    ctx, param = small()
    fj = L.to_jl(dc.feats_of(dc.n_images(K), 7))
    for alpha in (0.0, 1.0):
        ref = L.beam_nbest_batch(ctx, param, fj, K, NWORD, alpha)
        got = L.beam_diverse_batch(ctx, param, fj, K, 1, lam, NWORD, alpha)
        assert [img[0] for img in got] == ref and all(len(img) == 1 for img in got)


def test_one_group_is_nbest_bit_for_bit_bf16_production_route():
    P = production()
    N, K, nword = 512, 10, 8
    fj = L.to_jl(dc.feats_of(N, 11))
    ref = L.beam_nbest_batch(P["ctx"], P["param"], fj, K, nword, 1.0)
    got = L.beam_diverse_batch(P["ctx"], P["param"], fj, K, 1, 0.7, nword, 1.0)
    assert [img[0] for img in got] == ref


# ------------------------------------------------------------------------------------------------ 2. groups against the host restatement
@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: "L%d-K%d-G%d-lam%g-a%g" % c)
def test_small_f32_against_host(case):
    n_layers, K, G, lam, alpha = case
    m, feats = dc.case_inputs(case)
    ctx, param = small(n_layers)
    gpu = L.beam_diverse_batch(ctx, param, L.to_jl(feats), K, G, lam, NWORD, alpha)
    ref = dv.search(nb.OracleStep(orc, m, feats), len(feats), K, G, lam, NWORD, alpha)
    Kp = K // G
    for img in gpu:
        assert len(img) == G
        for grp in img:
            assert 1 <= len(grp) <= Kp
            assert all(grp[q][2] >= grp[q + 1][2] for q in range(len(grp) - 1))
            for toks, lp, sc in grp:
                assert toks[0] == lrcn_amd.BOS and (toks[-1] == lrcn_amd.EOS or len(toks) == NWORD + 2)
    frac = compare(groups_of(gpu), groups_of(ref), label="L%d K%d G%d lam%g a%g" % case)
    print("L%d K%d G%d lambda %g alpha %g: %.1f %% of entries exact" % (case + (100 * frac,)))
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 3. strength 0: every group repeats group 0
@pytest.mark.parametrize("K,G", [(6, 3), (8, 8), (32, 4)])
def test_strength_zero_repeats_group_zero(K, G):
    ctx, param = small()
    res = L.beam_diverse_batch(ctx, param, L.to_jl(dc.feats_of(dc.n_images(K), 5)), K, G, 0.0, NWORD, 1.0)
    for img in res:
        for grp in img[1:]:
            assert [e[0] for e in grp] == [e[0] for e in img[0]]
            for (_, lp, sc), (_, lp0, sc0) in zip(grp, img[0]):
                assert abs(lp - lp0) <= 1e-6 * (1 + abs(lp0)), (lp, lp0)
                assert abs(sc - sc0) <= 1e-6 * (1 + abs(sc0)), (sc, sc0)


# ------------------------------------------------------------------------------------------------ 4. logp is the caption's log-likelihood
def test_logp_equals_caption_score_under_a_penalty():
    m = dc.small_model()
    m.p["bout"][0, lrcn_amd.EOS] += 6.0   # captions that end in eos
    N, K, G = 8, 6, 3
    ctx = L.Context(dc.ES, dc.ES, dc.ES, dc.VS, max_B=N * K * 4, max_T=28, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(dc.feats_of(N, 5))
    res = L.beam_diverse_batch(ctx, param, fj, K, G, 2.0, NWORD, 1.0)
    zero = L.beam_diverse_batch(ctx, param, fj, K, G, 0.0, NWORD, 1.0)
    assert [[e[0] for e in grp] for img in res for grp in img[1:]] != [[e[0] for e in grp] for img in zero for grp in img[1:]]   # the penalty acts
    caps, img_of, lps, scs = [], [], [], []
    for n, groups in enumerate(res):
        for g, grp in enumerate(groups):
            for toks, lp, sc in grp:
                words = toks[1:-1]
                if toks[-1] == lrcn_amd.EOS and 1 <= len(words) <= 27:
                    caps.append(words); img_of.append(n); lps.append(lp); scs.append(sc)
    assert len(caps) >= N * G
    s = L.score_pairs(ctx, param, fj, caps, img_of, list(range(len(caps))))
    for c, sv, lp, sc in zip(caps, s, lps, scs):
        assert abs(lp - sv) <= 1e-4 * (1 + abs(sv)), (c, lp, sv)
        assert abs(sc - sv / (len(c) + 1)) <= 1e-4 * (1 + abs(sv)), (c, sc, sv)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. a large strength keeps the groups' words apart
@pytest.mark.parametrize("K,G", [(8, 8), (12, 4)])
def test_large_strength_keeps_words_apart(K, G):
    ctx, param = small()
    res = L.beam_diverse_batch(ctx, param, L.to_jl(dc.feats_of(8, 4)), K, G, 1e4, NWORD, 0.0)
    for n, img in enumerate(res):
        for pos in range(1, NWORD + 2):
            seen = {}
            for g, grp in enumerate(img):
                for w in {t[pos] for t, _, _ in grp if len(t) > pos and t[pos] != lrcn_amd.EOS}:
                    assert seen.setdefault(w, g) == g, (n, pos, w)


# ------------------------------------------------------------------------------------------------ 6. repeatability, independence, no trace
def test_repeatable_independent_and_leaves_the_other_beams_alone():
    ctx, param = small()
    N, K, G = 8, 6, 3
    feats = dc.feats_of(N, 3)
    fj = L.to_jl(feats)
    beam0 = L.beam_search_batch(ctx, param, fj, K, NWORD)
    nbest0 = L.beam_nbest_batch(ctx, param, fj, K, NWORD, 0.5)
    a = L.beam_diverse_batch(ctx, param, fj, K, G, 0.8, NWORD, 0.5)
    b = L.beam_diverse_batch(ctx, param, fj, K, G, 0.8, NWORD, 0.5)
    assert a == b
    sub = [2, 5, 6]
    c = L.beam_diverse_batch(ctx, param, L.to_jl(feats[sub]), K, G, 0.8, NWORD, 0.5)
    assert c == [a[i] for i in sub]
    assert L.beam_search_batch(ctx, param, fj, K, NWORD) == beam0
    assert L.beam_nbest_batch(ctx, param, fj, K, NWORD, 0.5) == nbest0


# ------------------------------------------------------------------------------------------------ 7. argument errors
def test_argument_errors_return_einval():
    N = 4
    ctx = L.Context(dc.ES, dc.ES, dc.ES, dc.VS, max_B=16, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(dc.small_model().p)
    fj = L.to_jl(dc.feats_of(N, 1))
    lib = _lib.lib()
    out = (C.c_int32 * (N * 40 * 300))()
    n = (C.c_int * (N * 40))()
    lp = (C.c_float * (N * 40))()
    sc = (C.c_float * (N * 40))()

    def call(N_, K, G, lam, nword=4, alpha=0.0, o=out, ln=n, feats=fj):
        return lib.lrcn_beam_diverse_batch(ctx._h, L._p9(param), L._ptr(feats) if feats is not None else None, N_, K, G, lam, nword, alpha, o, ln, lp, sc)

    assert call(N, 4, 2, 0.5) == 0
    before = list(out), list(n), list(lp), list(sc)
    bad = [(N, 4, 0, 0.5), (N, 4, -1, 0.5), (N, 4, 3, 0.5), (N, 4, 8, 0.5),           # G < 1, G not dividing K
           (N, 4, 2, -0.5), (N, 4, 2, float("nan")), (N, 4, 2, float("inf")),       # lambda negative or not finite
           (1, 33, 1, 0.5), (1, 33, 3, 0.5), (N, 6, 2, 0.5), (0, 4, 2, 0.5), (N, 0, 1, 0.5)]   # K > 32, N*K > max_B, N < 1, K < 1
    for args in bad:
        assert call(*args) == -1, args   # LRCN_EINVAL
        assert lib.lrcn_last_error(ctx._h)
    assert call(N, 4, 2, 0.5, nword=0) == -1 and call(N, 4, 2, 0.5, nword=257) == -1
    assert call(N, 4, 2, 0.5, alpha=-1.0) == -1 and call(N, 4, 2, 0.5, alpha=float("nan")) == -1
    assert call(N, 4, 2, 0.5, o=None) == -1 and call(N, 4, 2, 0.5, ln=None) == -1 and call(N, 4, 2, 0.5, feats=None) == -1
    assert (list(out), list(n), list(lp), list(sc)) == before   # a rejected call writes nothing
    assert lib.lrcn_beam_diverse_batch(ctx._h, L._p9(param), L._ptr(fj), N, 4, 4, 1.0, 4, 1.0, out, n, None, None) == 0
    assert call(N, 4, 2, 0.5) == 0
    assert (list(out), list(n), list(lp), list(sc)) == before   # and a valid call afterwards gives what it gave
    ctx.close()
