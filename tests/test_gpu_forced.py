"""GPU: forced-word beam search (lrcn_beam_forced_batch / lrcn_forced_topk_logits, include/lrcn_forced.h): the top-K kernel on given logits
against the host rules, exactly, on every Q rung, both sides of the ladder's boundaries and the general form; end to end on small f32 models
against the host restatement (tests/forced_ref.py); logp against lrcn_score_pairs; the early stop; no sets are the constrained call bit for
bit, on the f32 route and on the bf16 fused record route; the bf16 cell-epilogue route; argument errors; a used context."""
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
import constrained_ref as cr  # noqa: E402
import forced_ref as fr  # noqa: E402
import nbest_ref as nb  # noqa: E402
from test_gpu_constrained import BANNED, MIN_LEN, NGRAM  # noqa: E402
from test_gpu_nbest import compare, feats_of, small_model  # noqa: E402  (that file's comparison, tolerances and small model)

pytestmark = pytest.mark.gpu

N, NWORD = fr.E2E_N, fr.E2E_NWORD
EOS, BOS, UNK = lrcn_amd.EOS, lrcn_amd.BOS, lrcn_amd.UNK


def small_ctx(n_layers=2, max_B=256, max_T=2):
    return L.Context(64, 64, 64, 203, max_B=max_B, max_T=max_T, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)


def assert_meets_and_obeys(res, forced, banned, min_len, n, nword=NWORD):
    for img, sets in zip(res, forced):
        for toks, _, _ in img:
            assert toks[0] == BOS and fr.meets(toks, sets) and cr.obeys(toks, banned, min_len, n, nword), (toks, sets)


# ------------------------------------------------------------------------------------------------ 1. the kernel on given logits, exact
_logit_ctx = {}
_bf16 = {}


def logit_ctx():
    if not _logit_ctx:
        _logit_ctx["ctx"] = L.Context(16, 16, 16, 20, max_B=8, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)   # the entry does not depend on its sizes
    return _logit_ctx["ctx"]


def teardown_module(module):
    for d in (_logit_ctx, _bf16):
        if d:
            d["ctx"].close()
            d.clear()


def check_rows(ctx, z, K, hist, current, words, banned=(), min_len=0, n=0, label=""):
    """one call against the rules: stay columns and states exactly, the moves' -inf pattern exactly, values within 1e-5 (1 + |v|)"""
    hist = np.asarray(hist, np.int32)
    R, Cn, An = words.shape
    idx, lp, mv, st = L.forced_topk_logits(ctx, z, K, hist, current, words, banned, min_len, n)
    for r in range(R):
        h = [int(t) for t in hist[r, :current]]
        sets = [[int(w) for w in words[r, c]] for c in range(Cn)]
        cols, vals, moves = fr.proposals(nb.log_softmax(z[r]), K, h, current, sets, cr.banned_now(h, current, banned, min_len, n))
        assert int(st[r]) == fr.state_of(h, sets), (label, r, int(st[r]), fr.state_of(h, sets))
        assert list(idx[r]) == [int(c) for c in cols], (label, r, list(idx[r]), list(cols))
        assert np.all(np.abs(lp[r] - vals) <= 1e-5 * (1 + np.abs(vals))), (label, r, lp[r], vals)
        want = np.full(Cn * An, -np.inf, np.float32)
        for c, a, _, v in moves:
            want[c * An + a] = v
        assert np.array_equal(np.isinf(mv[r]), np.isinf(want)) and np.all(mv[r][np.isinf(want)] < 0), (label, r, mv[r], want)
        ok = ~np.isinf(want)
        assert np.all(np.abs(mv[r][ok] - want[ok]) <= 1e-5 * (1 + np.abs(want[ok]))), (label, r, mv[r], want)
    return idx, mv, st


def forced_rows_exact(V, K, Cn, An, plant=False):
    """The body of the two tests below.  Logits are multiples of 1/8 in [-16, 16.5] (given_logits_exact's construction in
    tests/test_gpu_constrained.py: equal logits give equal float logp and distinct ones differ by 0.125, far above the normaliser's
    rounding, so the ranking is (z descending, column ascending)).  Eos is the argmax of every row: rule 4 alone decides whether it leads.
    plant: forced words sit in the row's last two columns, which are also its best words, and on its best word below them."""
    R, CA = 8, Cn * An
    ctx = logit_ctx()
    rng = np.random.default_rng([V, K, Cn, An, int(plant)])
    z = (rng.integers(-128, 129, size=(R, V)) / 8.0).astype(np.float32)
    z[:, EOS] = 16.5
    if plant:
        z[:, V - 1] = 16.25
        z[:, V - 2] = 16.375
    inner = np.arange(3, V - 2)
    words = np.full((R, Cn, An), -1, np.int32)
    filler = np.zeros((R, 4), np.int32)
    for r in range(R):
        best = int(inner[np.argmax(z[r, 3:V - 2])])
        perm = [int(v) for v in rng.permutation(inner) if v != best]
        ids = perm[:CA]
        filler[r] = perm[CA:CA + 4]
        if plant:
            ids[0] = V - 1 if r % 2 == 0 else V - 2
            if CA >= 2:
                ids[CA - 1] = V - 2 if r % 2 == 0 else V - 1
            if CA >= 3:
                ids[An] = best
        words[r] = np.array(ids, np.int32).reshape(Cn, An)
    if An > 1:
        words[2, 0, An - 1] = -1       # a missing alternative
    if Cn > 1:
        words[5, Cn - 1, :] = -1       # an absent set: the row's full mask lacks its bit
    banned = sorted(set(int(v) for v in rng.permutation(inner)[:40]) - set(int(w) for w in words.ravel()) - set(int(f) for f in filler.ravel()))[:6] + [BOS, UNK]
    # histories of 5 words: rows 0, 4 hold no forced word; 1, 5 a word of set 0; 2, 6 the last word of every set; 3, 7 the first word of
    # every set, and stale tokens outside [0, V).  Position 1 repeats at the end, so with n = 2 the word at position 2 is banned by rule 3.
    hist = np.full((R, 8), BOS, np.int32)
    for r in range(R):
        f = filler[r]
        row = [f[0], f[1], f[2], f[3], f[0]]
        present = [[int(w) for w in words[r, c] if w >= 0] for c in range(Cn)]
        kind = r % 4
        if kind == 1 and present[0]:
            row[1] = present[0][0]
        elif kind == 2:
            for c, p in enumerate(present):
                if p:
                    row[1 + c] = p[-1]
        elif kind == 3:
            for c, p in enumerate(present):
                if p:
                    row[1 + c] = p[0]
            if Cn < 3:
                row[3] = -1 if r == 3 else V
        hist[r, 1:6] = row
    none = hist.copy()
    none[:, 1:] = BOS
    idx, mv, st = check_rows(ctx, z, K, none, 1, words, label="current 1")
    assert EOS not in idx   # every row has a set and nothing is met at step 1: no eos, although it is the argmax
    idx, mv, st = check_rows(ctx, z, K, hist, 6, words, label="states none, some, all")
    full = [fr.full_of([[int(w) for w in words[r, c]] for c in range(Cn)]) for r in range(R)]
    assert [int(s) for s in st[[0, 4]]] == [0, 0] and all(int(st[r]) == full[r] for r in (2, 3, 6, 7)), (st, full)
    for r in range(R):   # rule 4, spelled out: the accepting rows lead with eos, the others never propose it
        assert (idx[r][0] == EOS) == (int(st[r]) == full[r]) and (EOS in idx[r]) == (int(st[r]) == full[r]), (r, idx[r], st[r])
        open_words = [int(words[r, c, a]) for c in range(Cn) for a in range(An) if words[r, c, a] >= 0 and not (int(st[r]) >> c) & 1]
        assert not (set(int(c) for c in idx[r]) & set(open_words)), (r, idx[r], open_words)
    if plant:   # the last slot's columns: a move where their set is open (the value is the row's second or third best logp), a stay column where it is met
        for r in (0, 4):
            assert np.isfinite(mv[r][0]) and (V - 1 not in idx[r]) and (CA < 2 or V - 2 not in idx[r]), (r, mv[r], idx[r])
        if K >= 5 and CA >= 2:
            assert all({V - 1, V - 2} <= set(int(c) for c in idx[r]) for r in (2, 3, 6, 7) if full[r] == (1 << Cn) - 1), idx
    check_rows(ctx, z, K, hist, 6, words, banned=banned, label="static bans")
    idx, _, _ = check_rows(ctx, z, K, hist, 6, words, min_len=6, n=1, label="current <= min_len, n 1")
    assert EOS not in idx
    idx, _, _ = check_rows(ctx, z, K, hist, 6, words, banned=banned, min_len=5, n=2, label="rule 3 bans a met forced word")
    for r in (1, 2, 3, 5, 6, 7):   # position 2 holds a forced word of set 0 (if the row has one): met, so an ordinary column, and banned by n = 2
        if hist[r, 2] in words[r]:
            assert hist[r, 2] not in idx[r], (r, idx[r], hist[r])
    a = L.forced_topk_logits(ctx, z, K, hist, 6, words, banned, 2, 3)
    b = L.forced_topk_logits(ctx, z, K, hist, 6, words, banned, 2, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))   # two identical calls: identical bits


@pytest.mark.parametrize("CA", [(1, 1), (3, 4)])
@pytest.mark.parametrize("K", [1, 5, 16])
# V: off the grids of 4 and 32 (Q = 4); the first Q = 8 shape, with a partial last bitmap word; the first Q = 12 shape; the largest one-pass
# shape (Q = 16); the general form
@pytest.mark.parametrize("V", [203, 4100, 8196, 16384, 16390])
def test_kernel_on_given_logits_exact(V, K, CA):
    forced_rows_exact(V, K, CA[0], CA[1])


@pytest.mark.parametrize("CA", [(1, 1), (3, 4)])
@pytest.mark.parametrize("K", [1, 5, 16])
# both sides of every boundary of k_forced_topk_rows' ladder, q = ceil(V / 1024) <= 4 | 8 | 12 (| 16 above)
@pytest.mark.parametrize("V", [4096, 4097, 8192, 8193, 12288, 12289])
def test_kernel_on_given_logits_exact_at_the_ladder_boundaries(V, K, CA):
    forced_rows_exact(V, K, CA[0], CA[1], plant=True)


def test_kernel_without_sets_is_the_constrained_kernel():
    ctx = logit_ctx()
    rng = np.random.default_rng(5)
    z = (rng.integers(-128, 129, size=(8, 4100)) / 8.0).astype(np.float32)
    hist = np.concatenate([np.full((8, 1), BOS, np.int32), rng.integers(3, 7, size=(8, 8)).astype(np.int32)], axis=1)
    a = L.constrained_topk_logits(ctx, z, 5, hist, 9, (4, 9), 3, 2)
    for words in (np.zeros((8, 0, 1), np.int32), np.full((8, 2, 3), -1, np.int32)):   # C = 0; every set absent
        idx, lp, mv, st = L.forced_topk_logits(ctx, z, 5, hist, 9, words, (4, 9), 3, 2)
        assert idx.tobytes() == a[0].tobytes() and lp.tobytes() == a[1].tobytes() and not st.any() and np.all(np.isinf(mv))


# ------------------------------------------------------------------------------------------------ 2. end to end, f32, against the reference
_refs = {}


def reference(n_layers, C_, K, alpha, eos_bias=0.0, early_stop=True, min_len=MIN_LEN):
    key = (n_layers, C_, K, alpha, eos_bias, early_stop, min_len)
    if key not in _refs:
        m = small_model(n_layers=n_layers)
        m.p["bout"][0, EOS] += eos_bias
        _refs[key] = fr.search_forced(nb.OracleStep(orc, m, feats_of(N, fr.E2E_FEAT_SEED)), N, K, NWORD, alpha, fr.e2e_forced(C_),
                                      allowed=cr.hook(BANNED, min_len, NGRAM), early_stop=early_stop)
    return _refs[key]


@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("CK", fr.E2E_CASES)
def test_small_f32_against_host(n_layers, alpha, CK):
    """(tests/test_forced_host.py shows that the reference, perturbed by 1e-6, agrees with itself on all of these entries.)"""
    Cn, K = CK
    m = small_model(n_layers=n_layers)
    ctx = small_ctx(n_layers)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, fr.E2E_FEAT_SEED))
    forced = fr.e2e_forced(Cn)
    gpu = L.beam_forced_batch(ctx, param, fj, K, NWORD, alpha, forced, BANNED, MIN_LEN, NGRAM)
    free = L.beam_constrained_batch(ctx, param, fj, K, NWORD, alpha, BANNED, MIN_LEN, NGRAM)
    ctx.close()
    assert_meets_and_obeys(gpu, forced, BANNED, MIN_LEN, NGRAM)
    for n, g in enumerate(gpu):
        assert len(g) <= K and all(g[q][2] >= g[q + 1][2] for q in range(len(g) - 1))
        if forced[n]:
            assert [e[0] for e in g] != [e[0] for e in free[n]], n   # the sets bind
        else:
            assert [e[0] for e in g] == [e[0] for e in free[n]], n   # an image without sets: its n-best list
    frac = compare(gpu, reference(n_layers, Cn, K, alpha), label="forced L%d C%d K%d a%g" % (n_layers, Cn, K, alpha))
    print("forced f32 L%d C%d K%d alpha %g: %.1f %% of entries exact" % (n_layers, Cn, K, alpha, 100 * frac))
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 3. out_logp is the model's
def test_logp_equals_caption_score():
    m = small_model()
    m.p["bout"][0, EOS] += 6.0   # captions that end in eos
    K, Cn = 3, 2
    ctx = small_ctx(max_B=N * 4 * K, max_T=28)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 5))
    forced = fr.e2e_forced(Cn)
    res = L.beam_forced_batch(ctx, param, fj, K, NWORD, 1.0, forced, BANNED, 0, 2)
    assert_meets_and_obeys(res, forced, BANNED, 0, 2)
    caps, img, lps, scs = [], [], [], []
    for n, entries in enumerate(res):
        for toks, lp, sc in entries:
            words = toks[1:-1]
            if toks[-1] == EOS and 1 <= len(words) <= 27:
                caps.append(words); img.append(n); lps.append(lp); scs.append(sc)
    assert len(caps) >= N
    s = L.score_pairs(ctx, param, fj, caps, img, list(range(len(caps))))
    ctx.close()
    for c, sv, lp, sc in zip(caps, s, lps, scs):
        assert abs(lp - sv) <= 1e-4 * (1 + abs(sv)), (c, lp, sv)
        assert abs(sc - sv / (len(c) + 1)) <= 1e-4 * (1 + abs(sv)), (c, sc, sv)


# ------------------------------------------------------------------------------------------------ 4. the early stop stays exact
def test_early_stop_equals_the_full_run():
    m = small_model()
    m.p["bout"][0, EOS] += 6.0
    Cn, K, alpha = 2, 4, 0.0
    ctx = small_ctx()
    forced = fr.e2e_forced(Cn)
    gpu = L.beam_forced_batch(ctx, L.model_from_arrays(m.p), L.to_jl(feats_of(N, fr.E2E_FEAT_SEED)), K, NWORD, alpha, forced, BANNED, 4, NGRAM)
    ctx.close()
    assert_meets_and_obeys(gpu, forced, BANNED, 4, NGRAM)
    assert sum(1 for img in gpu for t, _, _ in img if t[-1] == EOS and len(t) < NWORD + 2) >= 1   # pools do fill before the length limit
    frac = compare(gpu, reference(2, Cn, K, alpha, eos_bias=6.0, early_stop=False, min_len=4), label="early stop")
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 5. no sets: the constrained call itself
def raw_call(ctx, param, fj, n_img, K, nword, alpha, cons, forced):
    lib = _lib.lib()
    out = (C.c_int32 * (n_img * K * (nword + 2)))()
    ln = (C.c_int * (n_img * K))()
    lp = (C.c_float * (n_img * K))()
    sc = (C.c_float * (n_img * K))()
    rc = lib.lrcn_beam_forced_batch(ctx._h, L._p9(param), L._ptr(fj), n_img, K, nword, alpha, C.byref(cons) if cons is not None else None,
                                    C.byref(forced) if forced is not None else None, out, ln, lp, sc)
    return rc, (bytes(out), bytes(ln), bytes(lp), bytes(sc))


def raw_constrained(ctx, param, fj, n_img, K, nword, alpha, cons):
    lib = _lib.lib()
    out = (C.c_int32 * (n_img * K * (nword + 2)))()
    ln = (C.c_int * (n_img * K))()
    lp = (C.c_float * (n_img * K))()
    sc = (C.c_float * (n_img * K))()
    rc = lib.lrcn_beam_constrained_batch(ctx._h, L._p9(param), L._ptr(fj), n_img, K, 0, 0.0, nword, alpha,
                                         C.byref(cons) if cons is not None else None, out, ln, lp, sc)
    return rc, (bytes(out), bytes(ln), bytes(lp), bytes(sc))


def no_sets_bit_for_bit(ctx, param, fj, n_img, K):
    arr = (C.c_int32 * 2)(*BANNED)
    for cons in (None, _lib.Constraints(arr, 2, MIN_LEN, NGRAM)):
        rc, ref = raw_constrained(ctx, param, fj, n_img, K, NWORD, 0.5, cons)
        assert rc == 0
        assert raw_call(ctx, param, fj, n_img, K, NWORD, 0.5, cons, None) == (0, ref)                       # forced == NULL
        assert raw_call(ctx, param, fj, n_img, K, NWORD, 0.5, cons, _lib.Forced(None, 0, 0)) == (0, ref)    # C == 0
    assert L.beam_forced_batch(ctx, param, fj, K, NWORD, 0.5) == L.beam_nbest_batch(ctx, param, fj, K, NWORD, 0.5)
    assert L.beam_forced_batch(ctx, param, fj, K, NWORD, 0.5, (), BANNED, MIN_LEN, NGRAM) == \
        L.beam_constrained_batch(ctx, param, fj, K, NWORD, 0.5, BANNED, MIN_LEN, NGRAM)


def test_no_sets_bit_for_bit_f32():
    ctx = small_ctx()
    no_sets_bit_for_bit(ctx, L.model_from_arrays(small_model().p), L.to_jl(feats_of(N, 3)), N, 5)
    ctx.close()


EB, VB, RB = 128, 520, 320   # bf16, 320 rows, H > 64, V % 4 == 0: the cell epilogue and tables, and at K < 6 the fused record route


def bf16():
    if not _bf16:
        m = orc.init_weights(EB, EB, EB, VB, seed=5)
        m.p["Wout"][:] *= 8.0
        _bf16.update(m=m, ctx=L.Context(EB, EB, EB, VB, max_B=RB, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16))
    return _bf16


def test_no_sets_bit_for_bit_bf16_record_route(monkeypatch):
    monkeypatch.delenv("LRCN_DECODE_SMAX", raising=False)
    B = bf16()
    no_sets_bit_for_bit(B["ctx"], L.model_from_arrays(B["m"].p), L.to_jl(feats_of(64, 2)), 64, 5)


def test_bf16_cell_epilogue_route_meets_and_obeys(monkeypatch):
    """32 images x 2 banks x 5: the 320 rows of that context, on the cell-epilogue and tables route; then 20 images x 4 banks x 4."""
    monkeypatch.delenv("LRCN_DECODE_SMAX", raising=False)
    B = bf16()
    ctx, param = B["ctx"], L.model_from_arrays(B["m"].p)
    for n_img, K, sets in ((32, 5, [[77, 300]]), (20, 4, [[77, 300], [5, 6, 7, 519]])):
        fj = L.to_jl(feats_of(n_img, 2))
        forced = [sets] * n_img
        res = L.beam_forced_batch(ctx, param, fj, K, NWORD, 1.0, sets, BANNED, 3, 2)
        assert_meets_and_obeys(res, forced, BANNED, 3, 2)
        assert all(1 <= len(img) <= K for img in res)
        assert res == L.beam_forced_batch(ctx, param, fj, K, NWORD, 1.0, forced, BANNED, 3, 2)   # per-image lists; a call repeats bit for bit
        assert res != L.beam_constrained_batch(ctx, param, fj, K, NWORD, 1.0, BANNED, 3, 2)


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors_return_einval():
    m = small_model()
    Vs, K, nword, n_img = 203, 3, 6, 2
    ctx = small_ctx(max_B=n_img * 8 * K)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(n_img, 1))
    lib = _lib.lib()

    def call(words, Cn, An, banned=(), min_len=0, n=0, K_=K, nword_=nword, alpha=0.0, null_words=False, n_img_=n_img):
        arr = (C.c_int32 * max(len(words), 1))(*words)
        ban = (C.c_int32 * max(len(banned), 1))(*banned)
        cons = _lib.Constraints(ban if banned else None, len(banned), min_len, n)
        return raw_call(ctx, param, fj, n_img_, K_, nword_, alpha, cons, _lib.Forced(None if null_words else arr, Cn, An))[0]

    good = [5, 6, 7, -1, 5, 6, 7, -1]   # two images x (C = 2, A = 2)
    assert call(good, 2, 2, banned=(9,), min_len=2, n=2) == 0
    most = list(range(10, 10 + Vs - 1 - nword - 4 - K))   # V - nbanned - 1 - nword - C*A == K: the largest feasible list
    assert call(good, 2, 2, banned=most) == 0
    bad = [
        dict(words=good, Cn=4, An=2), dict(words=good, Cn=-1, An=2), dict(words=good, Cn=2, An=0), dict(words=good, Cn=2, An=5),
        dict(words=good, Cn=2, An=2, null_words=True),
        dict(words=[5] * 16, Cn=3, An=1, K_=5),                               # 2^3 * 5 rows per image > 32
        dict(words=good * 3, Cn=2, An=2, n_img_=5),                           # N * S * K = 60 > max_B = 48 >= N * K (rejected before feats are read)
        dict(words=[5, 6, 7, 5, 6, 7], Cn=3, An=1, nword_=2),                 # nword < C
        dict(words=[5, EOS, 7, -1, 5, 6, 7, -1], Cn=2, An=2),                 # eos
        dict(words=[5, Vs, 7, -1, 5, 6, 7, -1], Cn=2, An=2),                  # >= V
        dict(words=[5, 6, 7, -1, 5, 6, 5, -1], Cn=2, An=2),                   # twice within image 1
        dict(words=good, Cn=2, An=2, banned=(9, 7)),                          # a forced word is banned
        dict(words=good, Cn=2, An=2, banned=most + [Vs - 1]),                 # feasibility
        dict(words=good, Cn=2, An=2, min_len=nword + 1), dict(words=good, Cn=2, An=2, n=-1),      # what lrcn_constraints checks
        dict(words=good, Cn=2, An=2, banned=(EOS,)), dict(words=good, Cn=2, An=2, banned=(9, 9)),
        dict(words=good, Cn=2, An=2, K_=0), dict(words=good, Cn=2, An=2, alpha=-1.0), dict(words=good, Cn=2, An=2, nword_=0),   # lrcn_beam_nbest_batch's
    ]
    for kw in bad:
        assert call(**kw) == -1, kw   # LRCN_EINVAL
        assert lib.lrcn_last_error(ctx._h)
    assert call([5, 6, 7, -1, 5, 6, 7, -1], 2, 2) == 0 and call([5, 5], 1, 1) == 0   # the same id in two images is fine
    # the logits entry
    z = np.zeros((2, 203), np.float32)
    hist = np.full((2, 4), BOS, np.int32)
    w = np.array([[[5, 6]], [[7, -1]]], np.int32)
    for current in (0, 5, 300):   # < 1, > ld_hist, > LRCN_BEAM_MAXLEN - 1
        with pytest.raises(_lib.LrcnError):
            L.forced_topk_logits(ctx, z, 3, np.full((2, 4 if current < 300 else 400), BOS, np.int32), current, w)
    for wbad in ([[[5, 5]], [[7, -1]]], [[[5, 0]], [[7, -1]]], [[[5, 203]], [[7, -1]]], np.zeros((2, 4, 1), np.int32) + 9, np.zeros((2, 1, 5), np.int32) - 1):
        with pytest.raises(_lib.LrcnError):
            L.forced_topk_logits(ctx, z, 3, hist, 2, np.asarray(wbad, np.int32))
    with pytest.raises(_lib.LrcnError):
        L.forced_topk_logits(ctx, z, 3, hist, 2, w, banned=[5])
    with pytest.raises(_lib.LrcnError):
        L.forced_topk_logits(ctx, z, 3, hist, 2, w, banned=list(range(8, 203)) + [1, 2])   # 203 - 197 - 1 - 1 - 2 = 2 < K
    idx, _, mv, st = L.forced_topk_logits(ctx, z, 3, hist, 2, w, banned=list(range(8, 203)) + [1])   # ... = 3: feasible
    assert [list(r) for r in idx] == [[2, 3, 4], [2, 3, 4]] and not st.any() and np.isinf(mv).tolist() == [[False, False], [False, True]]
    import torch
    zt = torch.zeros((2, 203), dtype=torch.float32, device="cuda:%d" % ctx.device)   # row stride 203: ld % 4 != 0
    with pytest.raises(_lib.LrcnError):
        L.forced_topk_logits(ctx, zt, 3, hist, 1, w)
    # the context is still usable
    assert call(good, 2, 2, banned=(9,), min_len=2, n=2) == 0
    assert L.beam_nbest_batch(ctx, param, fj, K, nword, 0.0)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. a used context
def test_used_context_repeats_bit_for_bit():
    m = small_model()
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 3))
    forced = fr.e2e_forced(2)
    ctx = small_ctx()
    a = L.beam_forced_batch(ctx, param, fj, 4, NWORD, 0.5, forced, BANNED, MIN_LEN, NGRAM)
    mid = L.beam_constrained_batch(ctx, param, fj, 4, NWORD, 0.5, BANNED, MIN_LEN, NGRAM)   # a constrained call after a forced call
    div = L.beam_diverse_batch(ctx, param, fj, 4, 2, 0.5, NWORD, 0.5)                        # (it shares the done flags)
    b = L.beam_forced_batch(ctx, param, fj, 4, NWORD, 0.5, forced, BANNED, MIN_LEN, NGRAM)
    wide = L.beam_forced_batch(ctx, param, fj, 4, NWORD, 0.5, fr.e2e_forced(3), BANNED, MIN_LEN, NGRAM)
    c = L.beam_forced_batch(ctx, param, fj, 4, NWORD, 0.5, forced, BANNED, MIN_LEN, NGRAM)   # after a call with more banks
    ctx.close()
    fresh = small_ctx()
    ref = L.beam_constrained_batch(fresh, param, fj, 4, NWORD, 0.5, BANNED, MIN_LEN, NGRAM)
    ref_div = L.beam_diverse_batch(fresh, param, fj, 4, 2, 0.5, NWORD, 0.5)
    fresh.close()
    assert a == b == c and mid == ref and div == ref_div and a != mid and wide != a
