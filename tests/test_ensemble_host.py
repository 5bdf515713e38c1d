"""CPU: the host restatement of the ensemble mixture (tests/ensemble_ref.py, include/lrcn_ensemble.h): PROB mixtures are normalised,
identical members reproduce the single member, the float32 restatement of the kernel's formula stays within the value tolerance of the
float64 definition over the GPU test's shapes, the searches agree entry for entry between the float32 and the float64 mix (on logit tables
and on the two oracle models of the GPU test, whose ensemble lists differ from each member's own), and the binding of the header (no GPU
call)."""
import os
import re
import sys

import numpy as np
import pytest

from lrcn_amd import _lib
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import constrained_ref as cr  # noqa: E402
import ensemble_ref as er  # noqa: E402
import nbest_ref as nb  # noqa: E402


def plain(pools):
    return [[(t, float(lp), float(sc)) for t, lp, sc in p] for p in pools]


@pytest.mark.parametrize("M", er.MIX_M)
def test_prob_mixtures_are_normalised_and_logprob_ones_are_not_above(M):
    for V in (20, 203, 1027):
        for scale in er.MIX_SCALES:
            zs, w = er.mix_inputs(V, M, scale)
            wn = er.weights(w, M)
            assert abs(float(wn.astype(np.float64).sum()) - 1.0) <= 1e-6
            x = er.mix(zs, wn, er.PROB)
            assert np.all(np.isfinite(x))   # the column at -1e4 in every member included
            assert np.all(np.abs(np.exp(x).sum(axis=1) - 1.0) <= 1e-6), (V, scale)   # (the float32 weights sum to 1 within 2^-23 M)
            g = er.mix(zs, wn, er.LOGPROB)
            assert np.all(np.isfinite(g)) and np.all(np.exp(g).sum(axis=1) <= 1.0 + 1e-6)   # weighted geometric <= arithmetic mean
            assert np.all(g <= x + 1e-9 * (1 + np.abs(x)))


@pytest.mark.parametrize("mode", [er.PROB, er.LOGPROB])
def test_identical_members_reproduce_the_single_member(mode):
    zs, _ = er.mix_inputs(203, 1, 8.0)
    one = er.log_softmax64(zs[0])
    for M in (1, 2, 3, 8):
        w = er.weights([m + 1.0 for m in range(M)], M)
        x = er.mix([zs[0]] * M, w, mode)
        assert er.mix_error(x, one) <= 1e-6, (M, er.mix_error(x, one))    # the float32 weights sum to 1 within 2^-23 M, times |lp| <= 1e4
        x32 = er.mix_f32([zs[0]] * M, w, mode)
        assert er.mix_error(x32, one) <= er.MIX_TOL, (M, er.mix_error(x32, one))
    # through the search: an ensemble of one table three times is the table
    step = nb.table_step(203, 2)
    ens = er.EnsembleStep([nb.table_step(203, 2)] * 3, None, mode)
    a, b = nb.search(ens, 3, 3, 6, 1.0), nb.search(step, 3, 3, 6, 1.0)
    assert [[e[0] for e in p] for p in a] == [[e[0] for e in p] for p in b]
    for p, q in zip(a, b):
        for (_, lp, _), (_, lq, _) in zip(p, q):
            assert abs(float(lp) - float(lq)) <= 1e-5 * (1 + abs(float(lq)))


@pytest.mark.parametrize("M", er.MIX_M)
@pytest.mark.parametrize("V", er.MIX_V)
def test_float32_formula_within_the_value_tolerance(V, M):
    worst = 0.0
    for scale in er.MIX_SCALES:
        zs, w = er.mix_inputs(V, M, scale)
        wn = er.weights(w, M)
        for mode in (er.PROB, er.LOGPROB):
            e = er.mix_error(er.mix_f32(zs, wn, mode), er.mix(zs, wn, mode))
            worst = max(worst, e)
            assert e <= er.MIX_TOL, (V, M, scale, mode, e)
    print("float32 formula V %d M %d: worst error %.3g of (1 + |v|)" % (V, M, worst))


@pytest.mark.parametrize("mode", [er.PROB, er.LOGPROB])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_searches_agree_between_the_float32_and_float64_mix_on_tables(K, alpha, mode):
    def members():
        return [nb.table_step(203, 11), nb.table_step(203, 12, scale=2.0)]
    a = nb.search(er.EnsembleStep(members(), er.E2E_W, mode), 8, K, 12, alpha)
    b = nb.search(er.EnsembleStep(members(), er.E2E_W, mode, mixer=er.mix_f32), 8, K, 12, alpha)
    assert [[e[0] for e in p] for p in a] == [[e[0] for e in p] for p in b]
    own = nb.search(members()[0], 8, K, 12, alpha)
    assert [[e[0] for e in p] for p in a] != [[e[0] for e in p] for p in own]   # the second member matters
    if K == 3:   # the constrained and the grouped search run on the wrapped step unchanged
        hook = cr.hook((122, 2), 3, 2)
        c = cr.search(er.EnsembleStep(members(), er.E2E_W, mode), 4, K, 12, alpha, allowed=hook)
        assert all(cr.obeys(t, (122, 2), 3, 2, 12) for p in c for t, _, _ in p)
        d = cr.search_diverse(er.EnsembleStep(members(), er.E2E_W, mode), 4, 6, 3, 0.5, 12, alpha, allowed=hook)
        assert all(len(img) == 3 and all(cr.obeys(t, (122, 2), 3, 2, 12) for g in img for t, _, _ in g) for img in d)


@pytest.mark.parametrize("mode", [er.PROB, er.LOGPROB])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_the_gpu_tests_reference_is_within_its_own_cap(K, alpha, mode):
    """The inputs of test_gpu_ensemble.test_small_f32_against_host: the float32-mix and float64-mix searches over the two oracle models
    agree entry for entry, so the reference alone uses none of the 5 % that test allows; and the ensemble's lists are neither member's."""
    ms, feats, N, nword = er.e2e_members(orc), er.e2e_feats(), er.E2E_N, er.E2E_NWORD

    def ens(mixer):
        return er.EnsembleStep([nb.OracleStep(orc, m, feats) for m in ms], er.E2E_W, mode, mixer=mixer)
    a = cr.search(ens(er.mix), N, K, nword, alpha)
    b = cr.search(ens(er.mix_f32), N, K, nword, alpha)
    assert [[e[0] for e in p] for p in a] == [[e[0] for e in p] for p in b]
    for m in ms:
        own = nb.search(nb.OracleStep(orc, m, feats), N, K, nword, alpha)
        assert [[e[0] for e in p] for p in a] != [[e[0] for e in p] for p in own]


def test_binding_declares_exactly_its_header():
    raw = open(_lib.ENSEMBLE_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_lib.ENSEMBLE_SIGNATURES) == ["lrcn_beam_ensemble_batch", "lrcn_ensemble_mix_logits"]
    assert "#define LRCN_ABI_VERSION" not in raw and '#include "lrcn_constrain.h"' in raw
    assert re.search(r"#define LRCN_ENSEMBLE_MAX 8\b", raw) and re.search(r"#define LRCN_ENSEMBLE_PROB 0\b", raw)
    assert re.search(r"#define LRCN_ENSEMBLE_LOGPROB 1\b", raw)
    header = open(_lib.HEADER).read()
    for name in names:
        assert name not in _lib.SIGNATURES and name not in header, name
        assert hasattr(_lib.lib(), name), name   # exported by the built library
