"""CPU: the host restatement of forced-word beam search (tests/forced_ref.py, include/lrcn_forced.h): without sets it is the constrained
search entry for entry; every entry meets its image's sets and obeys the constraints; the early stop equals the full run; a worked example
on a hand-written Markov model with its pools written out; the GPU test's cases agree with themselves under a 1e-6 perturbation of the
logits (so the reference alone uses none of the 5 % that test allows); and the binding of the header (no GPU call)."""
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
import forced_ref as fr  # noqa: E402
import nbest_ref as nb  # noqa: E402
from test_gpu_nbest import compare, feats_of, small_model  # noqa: E402  (that file's comparison and small model; nothing there runs on import)

BANNED, MIN_LEN, NGRAM = (122, 2), 3, 2   # the constraints of tests/test_gpu_constrained.py (2 = UNK)
N, NWORD = fr.E2E_N, fr.E2E_NWORD


def plain(pools):
    return [[(t, float(lp), float(sc)) for t, lp, sc in p] for p in pools]


def oracle_step(n_layers=2, eos_bias=0.0):
    m = small_model(n_layers=n_layers)
    m.p["bout"][0, nb.EOS] += eos_bias
    return nb.OracleStep(orc, m, feats_of(N, fr.E2E_FEAT_SEED))


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("K", [3, 5])
def test_no_sets_is_the_constrained_search(K, alpha):
    hook = cr.hook(BANNED, MIN_LEN, NGRAM)
    ref = plain(cr.search(oracle_step(), N, K, NWORD, alpha, allowed=hook))
    assert plain(fr.search_forced(oracle_step(), N, K, NWORD, alpha, [[] for _ in range(N)], allowed=hook)) == ref            # C = 0
    absent = [[[-1, -1], []] for _ in range(N)]                                                                              # C = 2, no id
    assert plain(fr.search_forced(oracle_step(), N, K, NWORD, alpha, absent, allowed=hook)) == ref
    assert plain(fr.search_forced(oracle_step(), N, K, NWORD, alpha, [[] for _ in range(N)])) == plain(cr.search(oracle_step(), N, K, NWORD, alpha))


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("C,K", fr.E2E_CASES)
def test_entries_meet_their_sets_and_obey_the_constraints(C, K, alpha):
    forced = fr.e2e_forced(C)
    hook = cr.hook(BANNED, MIN_LEN, NGRAM)
    res = fr.search_forced(oracle_step(), N, K, NWORD, alpha, forced, allowed=hook)
    free = cr.search(oracle_step(), N, K, NWORD, alpha, allowed=hook)
    for n in range(N):
        assert len(res[n]) <= K and all(res[n][q][2] >= res[n][q + 1][2] for q in range(len(res[n]) - 1))
        for toks, _, _ in res[n]:
            assert toks[0] == nb.BOS and fr.meets(toks, forced[n]) and cr.obeys(toks, BANNED, MIN_LEN, NGRAM, NWORD), (n, toks)
        if forced[n]:
            assert [e[0] for e in res[n]] != [e[0] for e in free[n]], n   # the sets bind
        else:
            assert plain([res[n]]) == plain([free[n]])                    # an image without sets is not touched by the others'
    assert sum(len(p) for p in res) >= N


@pytest.mark.parametrize("C,K", fr.E2E_CASES)
def test_early_stop_equals_the_full_run(C, K):
    forced = fr.e2e_forced(C)
    hook = cr.hook(BANNED, 4, NGRAM)
    a = fr.search_forced(oracle_step(eos_bias=6.0), N, K, NWORD, 0.0, forced, allowed=hook)
    b = fr.search_forced(oracle_step(eos_bias=6.0), N, K, NWORD, 0.0, forced, allowed=hook, early_stop=False)
    assert plain(a) == plain(b)
    assert sum(1 for p in a for t, _, _ in p if t[-1] == nb.EOS and len(t) < NWORD + 2) >= 1   # pools do fill before the length limit


# ------------------------------------------------------------------------------------------------ a worked example
# A Markov model over V = 8 tokens (0 eos, 1 bos): the logits depend on the last token alone and are multiples of 1/8.
MARKOV = {
    1: [-1.0, 0, 0, 1.0, 1.0, 2.0, 0, 0],      # after bos: 5 leads, the forced words 3 and 4 tie behind it
    3: [3.0, 0, 0, -2.0, 2.0, 1.0, 0, 0],      # after 3: eos, then 4, then 5
    4: [3.0, 0, 0, 2.0, -2.0, 1.0, 0, 0],      # after 4: eos, then 3, then 5
    5: [2.0, 0, 0, 1.5, 1.5, -2.0, 1.0, 0],    # after 5: eos, then 3 and 4
}
QUIET = [2.0, 0, 0, 0, 0, 0, 0, 0]             # after anything else: eos


def markov_step(req):
    z = np.array([MARKOV.get(int(tok), QUIET) for _, _, tok in req], np.float32)
    assert np.array_equal(z * 8, np.round(z * 8))
    return z, [None] * len(req)


def markov_logp(tokens):
    """the caption's log-probability from the table, in float64"""
    lp = 0.0
    for prev, tok in zip(tokens[:-1], tokens[1:]):
        z = np.array(MARKOV.get(prev, QUIET), np.float64)
        lp += z[tok] - z.max() - np.log(np.exp(z - z.max()).sum())
    return lp


def test_worked_example_on_a_markov_model():
    sets = [[3], [4]]   # both words must occur
    pools = fr.search_forced(markov_step, 1, 2, 4, 0.0, [sets])
    got = [t for t, _, _ in pools[0]]
    # Step 1: bank 00 keeps its two best stay columns 5 and 1 (3 and 4 are move words, eos is not allowed); banks 01 and 10 get [3] and [4].
    # Step 2: bank 11 is entered through both orders, [3 4] and [4 3], which tie; the lower candidate index ([3 4], from bank 01) leads.
    # Step 3: both end in eos at once (3.0 against 2.0 for going on) and fill the pool, in that order; nothing live can beat them.
    # By hand: log p = (1 - 2.8445) + (2 - 3.5360) + (3 - 3.5360) = -3.9165 for both.
    assert got == [[1, 3, 4, 0], [1, 4, 3, 0]], got
    for toks, lp, sc in pools[0]:
        assert abs(float(lp) - markov_logp(toks)) <= 1e-5 * (1 + abs(markov_logp(toks))) and float(sc) == float(lp)
        assert fr.meets(toks, sets) and abs(float(lp) + 3.9165) <= 1e-4
    assert plain(pools) == plain(fr.search_forced(markov_step, 1, 2, 4, 0.0, [sets], early_stop=False))
    # one set only: [3 .] at -2.3805, then [5 3 .] at -2.9809: 5 leads after bos, but it has to spend a step on 3
    one = fr.search_forced(markov_step, 1, 2, 4, 0.0, [[[3]]])
    assert [t for t, _, _ in one[0]] == [[1, 3, 0], [1, 5, 3, 0]], one
    # without sets the same model says [5]
    assert [t for t, _, _ in fr.search_forced(markov_step, 1, 2, 4, 0.0, [[]])[0]][0] == [1, 5, 0]
    # the states and the proposals of a row, spelled out
    assert fr.state_of([1, 5, 4], sets) == 2 and fr.state_of([1], sets) == 0 and fr.full_of(sets) == 3 and fr.full_of([[-1], [4]]) == 2
    cols, vals, moves = fr.proposals(nb.log_softmax(np.array(MARKOV[1], np.float32)), 2, [1], 1, sets)
    assert list(cols) == [5, 1] and [(c, a, w) for c, a, w, _ in moves] == [(0, 0, 3), (1, 0, 4)]
    cols, vals, moves = fr.proposals(nb.log_softmax(np.array(MARKOV[3], np.float32)), 2, [1, 3], 2, sets, ban={5})
    assert list(cols) == [1, 2] and [(c, a, w) for c, a, w, _ in moves] == [(1, 0, 4)]   # 3 is an ordinary column now; eos needs 4 first


# ------------------------------------------------------------------------------------------------ the GPU test's reference under perturbation
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("C,K", fr.E2E_CASES)
def test_the_gpu_tests_reference_is_within_its_own_cap(C, K, alpha, n_layers):
    """test_gpu_forced.test_small_f32_against_host allows 5 % of the entries to be logged near-ties.  The reference, run a second time with
    its logits moved by a fixed relative 1e-6 pattern, agrees with itself on at least 95 % of the entries by the same comparison."""
    forced, hook = fr.e2e_forced(C), cr.hook(BANNED, MIN_LEN, NGRAM)
    a = fr.search_forced(oracle_step(n_layers), N, K, NWORD, alpha, forced, allowed=hook)
    b = fr.search_forced(fr.perturbed(oracle_step(n_layers)), N, K, NWORD, alpha, forced, allowed=hook)
    frac = compare(plain(b), a, label="perturbed C%d K%d a%g L%d" % (C, K, alpha, n_layers))
    print("perturbed reference C %d K %d alpha %g L%d: %.1f %% of entries exact" % (C, K, alpha, n_layers, 100 * frac))
    assert frac >= 0.95, frac


def test_binding_declares_exactly_its_header():
    raw = open(_lib.FORCED_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_lib.FORCED_SIGNATURES) == ["lrcn_beam_forced_batch", "lrcn_forced_topk_logits"]
    assert "#define LRCN_ABI_VERSION" not in raw and '#include "lrcn_constrain.h"' in raw
    assert re.search(r"#define LRCN_FORCED_MAXSETS 3\b", raw) and re.search(r"#define LRCN_FORCED_MAXALT\s+4\b", raw)
    body = re.search(r"typedef struct \{(.*?)\} lrcn_forced;", txt, flags=re.S).group(1)
    fields = [d.strip().split()[-1].strip("*") for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.Forced._fields_], fields
    header = open(_lib.HEADER).read()
    for name in names:
        assert name not in _lib.SIGNATURES and name not in header, name
        assert hasattr(_lib.lib(), name), name   # exported by the built library
