"""CPU: the host restatement of diverse beam search (tests/diverse_ref.py, include/lrcn_diverse.h) on seeded random logit tables -- one
group is the n-best beam, the top-K window equals ranking the whole vocabulary, the per-image stop never changes the result, strength 0
repeats group 0, a large strength keeps the groups' words apart -- the stability of the inputs the GPU tests use, the host diversity
measures, and the library's export of lrcn_beam_diverse_batch (no GPU call)."""
import os
import re
import sys

import numpy as np
import pytest

import lrcn_amd  # noqa: F401
from lrcn_amd import _lib, diversity
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nbest_ref as nb  # noqa: E402
import diverse_ref as dv  # noqa: E402
import diverse_cases as dc  # noqa: E402

V, N, NWORD = 23, 3, 6
KG = [(4, 2), (6, 3), (6, 6), (8, 2), (12, 4)]
LAMBDAS = [0.0, 0.5, 2.0, 1e4]
QUANTA = [None, 0.5]


def flat(pools):
    return [[[(t, float(lp), float(sc)) for t, lp, sc in grp] for grp in img] for img in pools]


def table(seed, quantum, bonus=0.0):
    base = nb.table_step(V, seed, quantum=quantum)

    def step(req):
        z, h = base(req)
        z[:, nb.EOS] += np.float32(bonus)   # tables that favour eos fill the pools: groups get satisfied and images stop early
        return z, h
    return step


@pytest.mark.parametrize("quantum", QUANTA)
@pytest.mark.parametrize("K", [1, 3, 6])
def test_one_group_is_the_nbest_beam(K, quantum):
    for seed in range(4):
        for alpha in (0.0, 1.0):
            for lam in (0.0, 0.7):
                step = table(seed, quantum, bonus=seed % 3)
                a = dv.search(step, N, K, 1, lam, NWORD, alpha)
                b = nb.search(step, N, K, NWORD, alpha)
                assert flat(a) == flat([[p] for p in b])


@pytest.mark.parametrize("quantum", QUANTA)
@pytest.mark.parametrize("K,G", KG)
def test_window_equals_the_whole_vocabulary(K, G, quantum):
    for seed in range(2):
        for lam in LAMBDAS:
            step = table(seed, quantum, bonus=seed)
            assert flat(dv.search(step, N, K, G, lam, NWORD, 1.0, window=True)) == flat(dv.search(step, N, K, G, lam, NWORD, 1.0, window=False))


@pytest.mark.parametrize("quantum", QUANTA)
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K,G", KG)
def test_per_image_stop_never_changes_the_result(K, G, alpha, quantum):
    for lam in LAMBDAS:
        for seed in range(3):
            step = table(seed, quantum, bonus=1.5 * seed)
            a = dv.search(step, N, K, G, lam, NWORD, alpha, early_stop=True)
            b = dv.search(step, N, K, G, lam, NWORD, alpha, early_stop=False)
            assert flat(a) == flat(b)
            for img in a:
                assert len(img) == G
                for grp in img:
                    assert 1 <= len(grp) <= K // G
                    assert all(grp[q][2] >= grp[q + 1][2] for q in range(len(grp) - 1))
                    for toks, lp, sc in grp:
                        assert toks[0] == nb.BOS and (toks[-1] == nb.EOS or len(toks) == NWORD + 2)
                        assert sc == np.float32(lp / nb.length_factor(len(toks) - 1, alpha))


def test_the_stop_is_exercised():
    # the early exit is taken on eos-heavy tables: count the rows the callback is asked for
    calls = {True: 0, False: 0}
    for early in (True, False):
        base = table(1, None, bonus=4.0)

        def step(req, early=early):
            calls[early] += len(req)
            return base(req)
        dv.search(step, N, 6, 3, 0.5, NWORD, 0.0, early_stop=early)
    assert 0 < calls[True] < calls[False]


@pytest.mark.parametrize("quantum", QUANTA)
@pytest.mark.parametrize("K,G", KG)
def test_strength_zero_repeats_group_zero(K, G, quantum):
    for seed in range(3):
        res = flat(dv.search(table(seed, quantum, bonus=seed), N, K, G, 0.0, NWORD, 1.0))
        for img in res:
            assert all(grp == img[0] for grp in img)


@pytest.mark.parametrize("quantum", QUANTA)
@pytest.mark.parametrize("K,G", KG)
def test_large_strength_keeps_words_apart(K, G, quantum):
    # 1e4 outweighs every log-probability difference of these tables: a group takes a word that an earlier group holds at this position
    # only when it runs out of others (V - 1 = 22 non-eos words against at most K = 12 slots: never)
    for seed in range(3):
        res = dv.search(table(seed, quantum), N, K, G, 1e4, NWORD, 0.0)
        for img in res:
            for pos in range(1, NWORD + 2):
                seen = {}
                for g, grp in enumerate(img):
                    for w in {t[pos] for t, _, _ in grp if len(t) > pos and t[pos] != nb.EOS}:
                        assert seen.setdefault(w, g) == g, (seed, pos, w)


@pytest.mark.parametrize("case", dc.cases(), ids=lambda c: "L%d-K%d-G%d-lam%g-a%g" % c)
def test_gpu_case_inputs_are_stable(case):
    """Every case of test_gpu_diverse.py's comparison with this reference: the reference run twice, the second time with its logits scaled
    by (1 + 1e-6 u), u uniform in [-1, 1] -- about the disagreement a float32 GPU has with the oracle.  The two must agree on the tokens of
    >= 97.5 % of the entries (half the 5 % of near-ties that the GPU comparison allows); a case that does not gets another seed in
    diverse_cases.FEAT_SEED."""
    _, K, G, lam, alpha = case
    m, feats = dc.case_inputs(case)
    ref = dv.search(nb.OracleStep(orc, m, feats), len(feats), K, G, lam, dc.NWORD, alpha)
    inner = nb.OracleStep(orc, m, feats)
    rng = np.random.default_rng(11)

    def step(req):
        z, h = inner(req)
        return (z * (1.0 + 1e-6 * rng.uniform(-1.0, 1.0, z.shape))).astype(np.float32), h
    per = dv.search(step, len(feats), K, G, lam, dc.NWORD, alpha)
    entries = same = 0
    for a, b in zip(ref, per):
        for ga, gb in zip(a, b):
            entries += max(len(ga), len(gb))
            same += sum(x[0] == y[0] for x, y in zip(ga, gb))
    print("case %r: %d of %d entries agree" % (case, same, entries))
    assert same >= 0.975 * entries, (case, same, entries)


def test_distinct_n_and_overlap_by_hand():
    caps = [[5, 6, 7], [5, 6, 8], [9]]
    # unigrams: 5 6 7 5 6 8 9 -> 5 distinct of 7; bigrams: (5,6) (6,7) (5,6) (6,8) -> 3 of 4; no trigram repeats; nothing of length 4
    assert diversity.distinct_n(caps, 1) == 5 / 7
    assert diversity.distinct_n(caps, 2) == 3 / 4
    assert diversity.distinct_n(caps, 3) == 1.0
    assert diversity.distinct_n(caps, 4) == 0.0
    assert diversity.distinct_n([], 1) == 0.0
    # pairs: {5,6,7} {5,6,8} share 2 of 4; each with {9} shares 0 -> (0.5 + 0 + 0) / 3
    assert abs(diversity.mean_pairwise_overlap(caps) - 0.5 / 3) < 1e-15
    # bigram sets: {(5,6),(6,7)} {(5,6),(6,8)} -> 1 of 3; {9} has no bigram: 0 of 2, twice
    assert abs(diversity.mean_pairwise_overlap(caps, 2) - (1 / 3) / 3) < 1e-15
    assert diversity.mean_pairwise_overlap([[1, 2], [1, 2]]) == 1.0
    assert diversity.mean_pairwise_overlap([[1, 2]]) == 0.0
    assert diversity.distinct_n([["a", "dog"], ["a", "cat"]], 1) == 3 / 4   # words as well as ids


def test_signatures_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.DIVERSE_HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_lib.DIVERSE_SIGNATURES) == ["lrcn_beam_diverse_batch"]
    assert not set(names) & (set(_lib.SIGNATURES) | set(_lib.NBEST_SIGNATURES))
    res, args = _lib.DIVERSE_SIGNATURES["lrcn_beam_diverse_batch"]
    assert len(args) == 13
    assert '#include "lrcn_nbest.h"' in open(_lib.DIVERSE_HEADER).read()
    assert hasattr(_lib.lib(), "lrcn_beam_diverse_batch")   # exported by the built library


def test_generate_flags_parse():
    import importlib
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    o = cli.build_parser().parse_args(["--coco", "--generate", "20", "--nbest", "--beam_width", "6", "--diverse_groups", "3", "--diverse_strength", "0.8"])
    assert o.nbest and o.diverse_groups == 3 and abs(o.diverse_strength - 0.8) < 1e-12
    o = cli.build_parser().parse_args(["--coco", "--generate", "20", "--nbest"])
    assert o.diverse_groups == 0
