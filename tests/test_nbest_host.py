"""CPU: the host restatement of the n-best beam search (tests/nbest_ref.py) on seeded random logit tables -- the early stop never changes
the result, K = 1 at alpha 0 is greedy, the pool's tie and length-normalisation rules -- and the library's export of lrcn_beam_nbest_batch
(no GPU call)."""
import os
import re
import sys

import numpy as np
import pytest

import lrcn_amd  # noqa: F401
from lrcn_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nbest_ref as nb  # noqa: E402


def same(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert [(t, float(lp), float(sc)) for t, lp, sc in pa] == [(t, float(lp), float(sc)) for t, lp, sc in pb]


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("K", [1, 3, 10])
def test_early_stop_never_changes_the_result(alpha, K):
    stopped = 0
    for seed in range(6):
        V = 12 if K < 10 else 24
        base = nb.table_step(V, seed, scale=2.0 + seed % 3)

        def step(req, bonus=1.5 * (seed % 3)):   # some tables favour eos: pools fill and the bound stops images early
            z, h = base(req)
            z[:, nb.EOS] += bonus
            return z, h
        N, nword = 3, 6
        trace = []
        a = nb.search(step, N, K, nword, alpha, early_stop=True, trace=trace)
        b = nb.search(step, N, K, nword, alpha, early_stop=False)
        same(a, b)
        stopped += sum(1 for n in range(N) if max(s for i, s in trace if i == n) <= nword)
        for pool in a:
            assert 1 <= len(pool) <= K
            assert all(pool[q][2] >= pool[q + 1][2] for q in range(len(pool) - 1))
            for toks, lp, sc in pool:
                assert toks[0] == nb.BOS and (toks[-1] == nb.EOS or len(toks) == nword + 2)
                assert sc == np.float32(lp / nb.length_factor(len(toks) - 1, alpha))
    if K < 10 and alpha < 1.0:
        assert stopped > 0   # the test exercises the early exit


def test_eos_heavy_tables_stop_early_and_agree():
    # eos (column 0) made likely: the pools fill early and the bound stops images well before nword + 1
    base = nb.table_step(16, 99)

    def step(req):
        z, h = base(req)
        z[:, nb.EOS] += 3.0
        return z, h
    for alpha in (0.0, 0.7, 1.0):
        trace = []
        a = nb.search(step, 4, 4, 20, alpha, trace=trace)
        same(a, nb.search(step, 4, 4, 20, alpha, early_stop=False))
        assert max(s for _, s in trace) < 21


def test_k1_alpha0_is_greedy():
    for seed in range(8):
        step = nb.table_step(30, 1000 + seed)
        res = nb.search(step, 5, 1, 10, 0.0)
        g = nb.greedy(step, 5, 10)
        assert [pool[0][0] for pool in res] == g


def test_pool_ties_keep_insertion_order():
    pool = []
    for name, sc in [("a", -2.0), ("b", -1.0), ("c", -2.0), ("d", -1.0)]:
        nb.pool_insert(pool, 3, (name, np.float32(sc), np.float32(sc)))
    assert [e[0] for e in pool] == ["b", "d", "a"]          # equal scores: first inserted first; a full pool drops the last
    nb.pool_insert(pool, 3, ("e", np.float32(-2.0), np.float32(-2.0)))
    assert [e[0] for e in pool] == ["b", "d", "a"]          # equal to the worst: not strictly greater, stays out
    nb.pool_insert(pool, 3, ("f", np.float32(-1.5), np.float32(-1.5)))
    assert [e[0] for e in pool] == ["b", "d", "f"]


def _fixed_step(table):
    """logits from a dict history -> row (missing histories: a flat row)"""
    def step(req):
        out, hs = [], []
        for n, h, tok in req:
            hist = (h or ()) + (tok,)
            out.append(np.asarray(table.get(hist, [0.0, 0.0, 0.0, 0.0]), np.float32))
            hs.append(hist)
        return np.stack(out), hs
    return step


def test_length_normalisation_prefers_the_longer_caption():
    # after bos: eos at logp -0.85 (1 token) or word 2 then eos (2 tokens, total -1.03): the raw score takes the short caption, the score
    # per token (alpha 1) the longer one
    table = {(1,): [0.0, -9.0, 0.3, -9.0], (1, 2): [0.0, -9.0, -9.0, -0.5]}
    step = _fixed_step(table)
    raw = nb.search(step, 1, 2, 4, 0.0)[0]
    norm = nb.search(step, 1, 2, 4, 1.0)[0]
    lp_short = nb.log_softmax(np.float32([0.0, -9.0, 0.3, -9.0]))
    lp_long = lp_short[2] + nb.log_softmax(np.float32([0.0, -9.0, -9.0, -0.5]))[0]
    assert raw[0][0] == [1, 0] and float(raw[0][1]) == float(lp_short[0])
    assert norm[0][0] == [1, 2, 0] and float(norm[0][1]) == float(np.float32(lp_long))
    assert float(norm[0][2]) == float(np.float32(np.float32(lp_long) / np.float32(2.0)))


def test_finished_hypotheses_leave_the_beam():
    # K = 2: the eos candidate goes to the pool and is not extended; the beam continues with the other word, and a later entry displaces
    # only the pool's worst
    table = {(1,): [1.0, -9.0, 0.0, -9.0], (1, 2): [-9.0, -9.0, -9.0, 5.0], (1, 2, 3): [-9.0, -9.0, -9.0, 5.0],
             (1, 2, 3, 3): [-9.0, -9.0, -9.0, 5.0]}
    res = nb.search(_fixed_step(table), 1, 2, 3, 0.0)[0]
    assert [e[0] for e in res] == [[1, 0], [1, 2, 3, 3, 3]]


def test_signatures_match_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.NBEST_HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(_lib.NBEST_SIGNATURES) == ["lrcn_beam_nbest_batch"]
    assert not set(names) & set(_lib.SIGNATURES)      # lrcn.h and its symbols are unchanged
    res, args = _lib.NBEST_SIGNATURES["lrcn_beam_nbest_batch"]
    assert len(args) == 11


def test_generate_flags_parse():
    import importlib
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    o = cli.build_parser().parse_args(["--coco", "--generate", "20", "--nbest", "--beam_width", "4", "--length_norm", "0.7"])
    assert o.nbest and o.beam_width == 4 and abs(o.length_norm - 0.7) < 1e-12
    o = cli.build_parser().parse_args(["--coco", "--generate", "20"])
    assert not o.nbest and o.length_norm == 0.0
