"""CPU: the host restatement of constrained beam search (tests/constrained_ref.py, include/lrcn_constrain.h): with nothing constrained it is
nbest_ref.search / diverse_ref.search entry for entry; rule 3 against a brute-force enumeration of n-grams; on the small oracle model
every entry obeys the three rules and every image's list changes; exact ties (quantised logit tables); and the binding of the header
(no GPU call)."""
import os
import re
import sys

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import _lib
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import constrained_ref as cr  # noqa: E402
import diverse_ref as dv  # noqa: E402
import nbest_ref as nb  # noqa: E402

BANNED, MIN_LEN, NGRAM = (122, lrcn_amd.UNK), 3, 2   # the constraints of the small-model tests (here and in test_gpu_constrained.py)


def plain(pools):
    return [[(t, float(lp), float(sc)) for t, lp, sc in p] for p in pools]


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_empty_constraints_are_the_unconstrained_searches(K, alpha):
    for seed in range(3):
        step = nb.table_step(24, seed, scale=2.0 + seed)
        assert plain(cr.search(step, 3, K, 6, alpha)) == plain(nb.search(step, 3, K, 6, alpha))
        assert plain(cr.search(step, 3, K, 6, alpha, allowed=cr.hook())) == plain(nb.search(step, 3, K, 6, alpha))
    step = nb.table_step(24, 5)
    for K_, G in ((4, 2), (6, 3), (4, 1)):
        a = cr.search_diverse(step, 3, K_, G, 0.5, 6, alpha, allowed=cr.hook())
        b = dv.search(step, 3, K_, G, 0.5, 6, alpha)
        assert [plain(img) for img in a] == [plain(img) for img in b]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_rule_3_against_brute_force(n):
    rng = np.random.default_rng(n)
    hits = 0
    for _ in range(300):
        t = int(rng.integers(0, 40))
        hist = [nb.BOS] + [int(v) for v in rng.integers(3, 8, size=t)]   # a 5-word alphabet
        current = t + 1
        got = cr.banned_now(hist, current, (), 0, n)
        words = hist[1:]
        grams = {tuple(words[i:i + n]) for i in range(len(words) - n + 1)}    # every n-gram the history holds
        want = {v for v in range(0, 10) if t >= n - 1 and tuple(words[len(words) - (n - 1):] if n > 1 else []) + (v,) in grams}
        assert got == want, (hist, n, got, want)
        hits += bool(want)
    assert hits > 20   # the histories do repeat n-grams
    # rules 1 and 2 beside it
    assert cr.banned_now([nb.BOS, 5], 2, (7, 9), 2, 0) == {7, 9, nb.EOS}
    assert cr.banned_now([nb.BOS, 5, 6], 3, (7,), 2, 0) == {7}


def small_model(seed=3):
    m = orc.init_weights(64, 64, 64, 203, seed=seed)
    m.p["Wout"][:] *= 16.0
    return m


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", [3, 10])
def test_small_model_obeys_the_rules_and_every_list_changes(K, alpha):
    m, feats, N, nword = small_model(), feats_of(8, 7), 8, 12
    free = nb.search(nb.OracleStep(orc, m, feats), N, K, nword, alpha)
    con = cr.search(nb.OracleStep(orc, m, feats), N, K, nword, alpha, allowed=cr.hook(BANNED, MIN_LEN, NGRAM))
    ended = 0
    for n in range(N):
        assert 1 <= len(con[n]) <= K
        for toks, lp, sc in con[n]:
            assert cr.obeys(toks, BANNED, MIN_LEN, NGRAM, nword), (n, toks)
            ended += toks[-1] == nb.EOS
        assert [e[0] for e in con[n]] != [e[0] for e in free[n]], n
    print("K %d alpha %g: %d of %d entries end in eos" % (K, alpha, ended, sum(len(p) for p in con)))
    assert ended > 0


def test_exact_ties_on_quantised_tables():
    # logits on a grid of 0.5: exact ties in every row; the banned column's ties go to the next lower allowed column, deterministically
    step = nb.table_step(16, 4, scale=1.5, quantum=0.5)
    ban = (3, 4)
    a = cr.search(step, 4, 4, 6, 0.5, allowed=cr.hook(ban, 2, 2))
    b = cr.search(step, 4, 4, 6, 0.5, allowed=cr.hook(ban, 2, 2), early_stop=False)
    assert plain(a) == plain(b)   # the early stop stays exact under constraints
    for pool in a:
        for toks, _, _ in pool:
            assert cr.obeys(toks, ban, 2, 2, 6), toks
    lp = nb.log_softmax(np.array([1.0, 2.0, 2.0, 2.0, 0.5, 2.0], np.float32))
    cols, vals = cr.topk_allowed(lp, 3, {1, 7, -1})   # columns outside [0, V) are ignored
    assert list(cols) == [2, 3, 5] and vals[0] == vals[1] == vals[2] == lp[1]   # logp of the whole row: nothing is renormalised


def test_binding_declares_exactly_its_header():
    raw = open(_lib.CONSTRAIN_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_lib.CONSTRAIN_SIGNATURES) == ["lrcn_beam_constrained_batch", "lrcn_constrained_topk_logits"]
    assert "#define LRCN_ABI_VERSION" not in raw and '#include "lrcn_diverse.h"' in raw
    body = re.search(r"typedef struct \{(.*?)\} lrcn_constraints;", txt, flags=re.S).group(1)
    fields = [d.strip().split()[-1].strip("*") for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.Constraints._fields_], fields
    header = open(_lib.HEADER).read()
    for name in names:
        assert name not in _lib.SIGNATURES and name not in header, name
        assert hasattr(_lib.lib(), name), name   # exported by the built library
