"""GPU: constrained beam search (lrcn_beam_constrained_batch / lrcn_constrained_topk_logits, include/lrcn_constrain.h): the kernel on given
logits against the host rules, exactly, on every Q rung and the general form; end to end on small f32 models against the host restatement
(tests/constrained_ref.py); logp against lrcn_score_pairs; empty constraints are the unconstrained calls bit for bit, on the f32 route and on
the bf16 fused record route; constraints that cannot bind are the f32-logits route bit for bit on the bf16 cell-epilogue route; diverse
groups; the early stop; argument errors; a used context."""
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
import nbest_ref as nb  # noqa: E402
from test_gpu_nbest import compare, feats_of, small_model  # noqa: E402  (that file's comparison, tolerances and small model)

pytestmark = pytest.mark.gpu

BANNED, MIN_LEN, NGRAM = (122, lrcn_amd.UNK), 3, 2   # the constraints of tests/test_constrained_host.py
N, NWORD = 8, 12
EOS, BOS = lrcn_amd.EOS, lrcn_amd.BOS


def small_ctx(n_layers=2, max_B=N * 10, max_T=2):
    return L.Context(64, 64, 64, 203, max_B=max_B, max_T=max_T, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)


def assert_obeys(res, banned, min_len, n, nword=NWORD):
    for img in res:
        for toks, _, _ in img:
            assert toks[0] == BOS and cr.obeys(toks, banned, min_len, n, nword), toks


# ------------------------------------------------------------------------------------------------ 1. the kernel on given logits, exact
_logit_ctx = {}


def logit_ctx():
    if not _logit_ctx:
        _logit_ctx["ctx"] = L.Context(16, 16, 16, 20, max_B=8, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)   # the entry does not depend on its sizes
    return _logit_ctx["ctx"]


def teardown_module(module):
    for d in (_logit_ctx, _bf16):
        if d:
            d["ctx"].close()
            d.clear()


def check_rows(ctx, z, K, hist, current, banned=(), min_len=0, n=0, label=""):
    """one call against the rules: columns exactly, logp within 1e-5 (1 + |v|) (test_gpu_nbest.compare's tolerance)"""
    hist = np.asarray(hist, np.int32)
    idx, lp = L.constrained_topk_logits(ctx, z, K, hist, current, banned, min_len, n)
    for r in range(z.shape[0]):
        ban = cr.banned_now([int(t) for t in hist[r, :current]], current, banned, min_len, n)
        cols, vals = cr.topk_allowed(nb.log_softmax(z[r]), K, ban)
        assert list(idx[r]) == [int(c) for c in cols], (label, r, list(idx[r]), list(cols))
        assert np.all(np.abs(lp[r] - vals) <= 1e-5 * (1 + np.abs(vals))), (label, r, lp[r], vals)
        assert not (set(int(c) for c in idx[r]) & ban), (label, r)
    return idx, lp


def given_logits_exact(V, K, plant_last=False):
    """The body of the two tests below.  plant_last: the two best columns of every row are the row's last two (see the second test)."""
    R = 7
    ctx = logit_ctx()
    rng = np.random.default_rng([V, K])
    # multiples of 1/8 in [-16, 16]: many exact ties; equal logits give equal float logp and distinct ones differ by 0.125, far above the
    # normaliser's rounding on either side, so the ranking is (z descending, column ascending)
    z = (rng.integers(-128, 129, size=(R, V)) / 8.0).astype(np.float32)
    bos = np.full((R, 1), BOS, np.int32)
    top = [int(np.argmax(z[r])) for r in range(R)]   # before planting: the word-edge call below bans V - 1 and these, never V - 2
    if plant_last:
        mx = z.max(axis=1)
        z[:, V - 1] = mx + 0.125
        z[:, V - 2] = mx + 0.25
        assert float(z.max()) <= 16.25 and np.array_equal(z * 8, np.round(z * 8))   # still multiples of 1/8: the ranking argument holds
        assert all(V - 2 != t for t in top)
    idx, _ = check_rows(ctx, z, K, bos, 1, label="no constraint")
    if plant_last:   # what the host rules give, spelled out: the last slot's two columns lead every row
        assert all(list(idx[r][:2]) == [V - 2, V - 1][:K] for r in range(R)), idx[:, :2]
    check_rows(ctx, z, K, bos, 1, n=1, min_len=0, label="current 1, n 1")
    check_rows(ctx, z, K, bos, 1, min_len=1, label="current 1, eos banned")
    idx, _ = check_rows(ctx, z, K, bos, 1, banned=sorted({1, 31, 32, V - 1} | {t for t in top if t != EOS}),
                        label="bans on word edges and every argmax")
    if plant_last:   # V - 1 banned, V - 2 left: one of the last slot's two columns masked, the other the winner
        assert all(idx[r][0] == V - 2 and V - 1 not in idx[r] for r in range(R)), idx[:, 0]
    # exactly K columns left: every word but K + 2 kept ones is on the list (nbanned = V - K - current, current = 3), eos falls to min_len and
    # the two history words -- kept ones -- to n = 1
    keep = sorted(int(v) for v in rng.choice(np.arange(1, V), size=K + 2, replace=False))
    hist = np.array([[BOS, keep[0], keep[1]]] * R, np.int32)
    kept = set(keep)
    ban = [v for v in range(1, V) if v not in kept]
    assert len(ban) == V - K - 3
    idx, _ = check_rows(ctx, z, K, hist, 3, banned=ban, min_len=3, n=1, label="exactly K left")
    assert all(sorted(idx[r]) == keep[2:] for r in range(R))
    # eos the argmax: banned while current <= min_len, the winner at current = min_len + 1
    ze = z.copy()
    ze[:, EOS] = float(z.max()) + 0.5 if plant_last else 16.0   # (planted rows reach 16.25)
    h3 = np.array([[BOS, 5, 6]] * R, np.int32)
    idx, _ = check_rows(ctx, ze, K, h3, 2, min_len=2, label="eos argmax, current = min_len")
    assert EOS not in idx
    idx, _ = check_rows(ctx, ze, K, h3, 3, min_len=2, label="eos argmax, current = min_len + 1")
    assert all(idx[r][0] == EOS for r in range(R))
    # histories over a small alphabet (they repeat n-grams); n = 1, 2, 3 and n > current
    hr = np.concatenate([bos, rng.integers(3, 7, size=(R, 8)).astype(np.int32)], axis=1)
    for n in (1, 2, 3, 12):
        check_rows(ctx, z, K, hr, 9, n=n, banned=(top[0],) if top[0] != EOS else (), label="n = %d" % n)
    a = L.constrained_topk_logits(ctx, z, K, hr, 9, (4,), 0, 2)
    b = L.constrained_topk_logits(ctx, z, K, hr, 9, (4,), 0, 2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()   # two identical calls: identical bits
    # a suffix that occurs three times with three different continuations (each row's three best columns, so the bans bind)
    order = [[int(c) for c in nb.topk(nb.log_softmax(z[r]), 5)[0] if c != EOS][:3] for r in range(R)]
    h = np.array([[BOS, 9, 8, o[0], 9, 8, o[1], 9, 8, o[2], 9, 8] for o in order], np.int32)
    idx, _ = check_rows(ctx, z, K, h, 12, n=3, label="three continuations")
    assert all(not (set(idx[r]) & set(order[r])) for r in range(R))
    # tokens outside [0, V) in the history are ignored (n = 2: the suffix -1 was followed by 7; n = 1: every word used)
    h = np.array([[BOS, 5, -1, 7, V, 5, -1]] * R, np.int32)
    check_rows(ctx, z, K, h, 7, n=2, label="stale tokens, n 2")
    check_rows(ctx, z, K, h, 7, n=1, label="stale tokens, n 1")


@pytest.mark.parametrize("K", [1, 5, 32])
# V: off the grids of 4 and 32 (Q = 4); the first Q = 8 shape, with a partial last bitmap word; the first Q = 12 shape; the largest one-pass
# shape (Q = 16); the general form
@pytest.mark.parametrize("V", [203, 4100, 8196, 16384, 16390])
def test_kernel_on_given_logits_exact(V, K):
    given_logits_exact(V, K)


@pytest.mark.parametrize("K", [1, 32])
# V: both sides of every boundary of k_constrained_topk_rows' ladder, q = ceil(V / 1024) <= 4 | 8 | 12 (| 16: 16384 | 16390 above).  At
# V = 1024 Q the last column is thread 255's fourth element of slot Q - 1; at 1024 Q + 1 it is thread 0's first element of slot Q, the only
# live element of that slot, in a bitmap word of its own.
@pytest.mark.parametrize("V", [4096, 4097, 8192, 8193, 12288, 12289])
def test_kernel_on_given_logits_exact_at_the_ladder_boundaries(V, K):
    """The same calls with the decisive columns in the last slot: z[:, V - 2] and z[:, V - 1] are the row maximum + 0.25 and + 0.125, and the
    word-edge call bans V - 1.  A rung that drops or mis-masks its last slot fails on the column list.

    A local build (not kept) whose constrained_topk_rows_kernel<8> did not load its last slot failed [8192-1] and [8192-32] at the first
    call (column 259 for 8190; the list without 8190 and 8191) and passed everything else, test_kernel_on_given_logits_exact included: at
    V = 4097 and 4100 slot 7 holds no column, and the other widths are other instantiations."""
    given_logits_exact(V, K, plant_last=True)


# ------------------------------------------------------------------------------------------------ 2. end to end, f32, against the reference
_refs = {}


def reference(n_layers, K, alpha, eos_bias=0.0, early_stop=True, banned=BANNED, min_len=MIN_LEN, n=NGRAM, feat_seed=7):
    key = (n_layers, K, alpha, eos_bias, early_stop, banned, min_len, n, feat_seed)
    if key not in _refs:
        m = small_model(n_layers=n_layers)
        m.p["bout"][0, EOS] += eos_bias
        _refs[key] = cr.search(nb.OracleStep(orc, m, feats_of(N, feat_seed)), N, K, NWORD, alpha, allowed=cr.hook(banned, min_len, n),
                               early_stop=early_stop)
    return _refs[key]


@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("K", [3, 10])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_small_f32_against_host(n_layers, K, alpha):
    m = small_model(n_layers=n_layers)
    ctx = small_ctx(n_layers)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 7))
    gpu = L.beam_constrained_batch(ctx, param, fj, K, NWORD, alpha, BANNED, MIN_LEN, NGRAM)
    free = L.beam_nbest_batch(ctx, param, fj, K, NWORD, alpha)
    ctx.close()
    assert_obeys(gpu, BANNED, MIN_LEN, NGRAM)
    for g in gpu:
        assert 1 <= len(g) <= K and all(g[q][2] >= g[q + 1][2] for q in range(len(g) - 1))
    if n_layers == 2:
        for n in range(N):
            assert [e[0] for e in gpu[n]] != [e[0] for e in free[n]], n   # the constraints bind on every image
    frac = compare(gpu, reference(n_layers, K, alpha), label="constrained L%d K%d a%g" % (n_layers, K, alpha))
    print("constrained f32 L%d K%d alpha %g: %.1f %% of entries exact" % (n_layers, K, alpha, 100 * frac))
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 3. out_logp is the model's
def test_logp_equals_caption_score_under_bans():
    m = small_model()
    m.p["bout"][0, EOS] += 6.0   # captions that end in eos
    K = 3
    ctx = small_ctx(max_B=N * K * 4, max_T=28)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 5))
    res = L.beam_constrained_batch(ctx, param, fj, K, NWORD, 1.0, BANNED, 0, 2)
    assert_obeys(res, BANNED, 0, 2)
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


# ------------------------------------------------------------------------------------------------ 4. empty constraints are the existing calls
def test_empty_constraints_bit_for_bit_f32():
    m = small_model()
    ctx = small_ctx()
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 3))
    assert L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 0.5) == L.beam_nbest_batch(ctx, param, fj, 5, NWORD, 0.5)
    assert L.beam_constrained_batch(ctx, param, fj, 4, NWORD, 0.5, groups=2, strength=0.8) == L.beam_diverse_batch(ctx, param, fj, 4, 2, 0.8, NWORD, 0.5)
    lib = _lib.lib()   # cons == NULL as well
    out = (C.c_int32 * (N * 5 * (NWORD + 2)))()
    ln = (C.c_int * (N * 5))()
    assert lib.lrcn_beam_constrained_batch(ctx._h, L._p9(param), L._ptr(fj), N, 5, 0, 0.0, NWORD, 0.5, None, out, ln, None, None) == 0
    ref = L.beam_nbest_batch(ctx, param, fj, 5, NWORD, 0.5)
    toks = np.ctypeslib.as_array(out).reshape(N * 5, NWORD + 2)
    assert [[list(toks[r][:ln[r]]) for r in range(i * 5, i * 5 + 5) if ln[r]] for i in range(N)] == [[e[0] for e in img] for img in ref]
    ctx.close()


_bf16 = {}
EB, VB, RB = 128, 520, 320   # bf16, 320 rows, H > 64, V % 4 == 0: the cell epilogue and tables, and at K < 6 the fused record route


def bf16():
    if not _bf16:
        m = orc.init_weights(EB, EB, EB, VB, seed=5)
        m.p["Wout"][:] *= 8.0
        _bf16.update(m=m, ctx=L.Context(EB, EB, EB, VB, max_B=RB, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16))
    return _bf16


def test_empty_constraints_bit_for_bit_bf16_record_route(monkeypatch):
    monkeypatch.delenv("LRCN_DECODE_SMAX", raising=False)
    B = bf16()
    ctx, param = B["ctx"], L.model_from_arrays(B["m"].p)
    fj = L.to_jl(feats_of(64, 2))
    assert L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 1.0) == L.beam_nbest_batch(ctx, param, fj, 5, NWORD, 1.0)
    fj = L.to_jl(feats_of(80, 2))   # two groups need an even width: 80 images x 4 beams, the same 320 rows
    assert L.beam_constrained_batch(ctx, param, fj, 4, NWORD, 1.0, groups=2, strength=0.5) == L.beam_diverse_batch(ctx, param, fj, 4, 2, 0.5, NWORD, 1.0)


# ------------------------------------------------------------------------------------------------ 5. the constrained path on the bf16 epilogue routes
def test_bf16_cell_epilogue_route_nonbinding_then_binding(monkeypatch):
    B = bf16()
    m = B["m"]
    dead = 77
    saved = m.p["bout"][0, dead]
    m.p["bout"][0, dead] = -1e4   # a word no row proposes: banning it cannot bind
    ctx, param = B["ctx"], L.model_from_arrays(m.p)
    m.p["bout"][0, dead] = saved
    fj = L.to_jl(feats_of(64, 2))
    monkeypatch.delenv("LRCN_DECODE_SMAX", raising=False)
    con = L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 1.0, (dead,), 0, NWORD + 2)
    monkeypatch.setenv("LRCN_DECODE_SMAX", "0")
    rows = L.beam_nbest_batch(ctx, param, fj, 5, NWORD, 1.0)
    monkeypatch.delenv("LRCN_DECODE_SMAX")
    assert con == rows   # the same logits, the same normaliser arithmetic: the same bits
    count = {}
    for img in rows:
        for toks, _, _ in img:
            for t in toks[1:]:
                if t != EOS:
                    count[t] = count.get(t, 0) + 1
    ban = tuple(sorted(count, key=lambda t: (-count[t], t))[:2])
    res = L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 1.0, ban, 3, 2)
    assert_obeys(res, ban, 3, 2)
    assert all(len(img) >= 1 for img in res) and res != rows


# ------------------------------------------------------------------------------------------------ 6. diverse
def test_one_group_is_the_nbest_form_bit_for_bit():
    m = small_model()
    ctx = small_ctx()
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 3))
    a = L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 0.5, BANNED, MIN_LEN, NGRAM)
    b = L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 0.5, BANNED, MIN_LEN, NGRAM, groups=1, strength=0.7)
    ctx.close()
    assert [[img] for img in a] == b


def test_two_groups_against_host():
    m = small_model()
    K, G, lam, alpha = 4, 2, 0.5, 1.0
    ctx = small_ctx()
    feats = feats_of(N, 7)
    gpu = L.beam_constrained_batch(ctx, L.model_from_arrays(m.p), L.to_jl(feats), K, NWORD, alpha, BANNED, MIN_LEN, NGRAM, groups=G, strength=lam)
    ctx.close()
    ref = cr.search_diverse(nb.OracleStep(orc, m, feats), N, K, G, lam, NWORD, alpha, allowed=cr.hook(BANNED, MIN_LEN, NGRAM))
    for img in gpu:
        assert len(img) == G
        assert_obeys(img, BANNED, MIN_LEN, NGRAM)
    frac = compare([g for img in gpu for g in img], [g for img in ref for g in img], label="constrained diverse")
    print("constrained diverse: %.1f %% of entries exact" % (100 * frac))
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 7. the early stop stays exact
def test_early_stop_equals_the_full_run():
    m = small_model()
    m.p["bout"][0, EOS] += 6.0
    K, alpha = 3, 0.0
    ctx = small_ctx()
    gpu = L.beam_constrained_batch(ctx, L.model_from_arrays(m.p), L.to_jl(feats_of(N, 7)), K, NWORD, alpha, BANNED, 4, NGRAM)
    ctx.close()
    assert_obeys(gpu, BANNED, 4, NGRAM)
    assert sum(1 for img in gpu for t, _, _ in img if t[-1] == EOS and len(t) < NWORD + 2) >= 1   # pools do fill before the length limit
    ref = reference(2, K, alpha, eos_bias=6.0, early_stop=False, min_len=4)
    frac = compare(gpu, ref, label="early stop")
    assert frac >= 0.95, frac


# ------------------------------------------------------------------------------------------------ 8. argument errors
def test_argument_errors_return_einval():
    m = small_model()
    Vs, K, nword, n_img = 203, 3, 6, 2
    ctx = small_ctx()
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(n_img, 1))
    lib = _lib.lib()
    out = (C.c_int32 * (n_img * K * (nword + 2)))()
    ln = (C.c_int * (n_img * K))()

    def call(ids, min_len=0, n=0, null_list=False):
        arr = (C.c_int32 * max(len(ids), 1))(*ids)
        cons = _lib.Constraints(None if null_list else arr, len(ids), min_len, n)
        return lib.lrcn_beam_constrained_batch(ctx._h, L._p9(param), L._ptr(fj), n_img, K, 0, 0.0, nword, 0.0, C.byref(cons), out, ln, None, None)

    assert call([5, 6], 2, 2) == 0
    most = list(range(1, 1 + Vs - 1 - nword - K))   # V - nbanned - 1 - nword == K: the largest feasible list
    assert call(most) == 0
    for args in [([EOS],), ([Vs],), ([-3],), ([5, 9, 5],), ([], nword + 1), ([], -1), ([], 0, -1), (most + [Vs - 1],), ([5], 0, 0, True)]:
        assert call(*args) == -1, args   # LRCN_EINVAL
        assert lib.lrcn_last_error(ctx._h)
    bad = _lib.Constraints(None, -1, 0, 0)
    assert lib.lrcn_beam_constrained_batch(ctx._h, L._p9(param), L._ptr(fj), n_img, K, 0, 0.0, nword, 0.0, C.byref(bad), out, ln, None, None) == -1
    assert lib.lrcn_beam_constrained_batch(ctx._h, L._p9(param), L._ptr(fj), n_img, K, -1, 0.0, nword, 0.0, None, out, ln, None, None) == -1
    # the logits entry
    import torch
    z = torch.zeros((2, 203), dtype=torch.float32, device="cuda:%d" % ctx.device)   # row stride 203: ld % 4 != 0
    hist = np.full((2, 4), BOS, np.int32)
    with pytest.raises(_lib.LrcnError):
        L.constrained_topk_logits(ctx, z, 3, hist, 1)
    z = np.zeros((2, 203), np.float32)
    for current in (0, 5, 300):   # < 1, > ld_hist, > LRCN_BEAM_MAXLEN - 1
        with pytest.raises(_lib.LrcnError):
            L.constrained_topk_logits(ctx, z, 3, np.full((2, 4 if current < 300 else 400), BOS, np.int32), current)
    with pytest.raises(_lib.LrcnError):
        L.constrained_topk_logits(ctx, z, 3, hist, 2, banned=list(range(1, 200)))   # 203 - 199 - 1 - 1 = 2 < K
    idx, _ = L.constrained_topk_logits(ctx, z, 3, hist, 2, banned=list(range(1, 199)))   # ... = 3: feasible
    assert [list(r) for r in idx] == [[0, 199, 200]] * 2
    # the context is still usable
    assert call([5, 6], 2, 2) == 0
    assert L.beam_nbest_batch(ctx, param, fj, K, nword, 0.0)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 9. a used context
def test_used_context_repeats_bit_for_bit():
    m = small_model()
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 3))
    ctx = small_ctx()
    a = L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 0.5, BANNED, MIN_LEN, NGRAM)
    mid = L.beam_nbest_batch(ctx, param, fj, 5, NWORD, 0.5)
    b = L.beam_constrained_batch(ctx, param, fj, 5, NWORD, 0.5, BANNED, MIN_LEN, NGRAM)
    ctx.close()
    fresh = small_ctx()
    ref = L.beam_nbest_batch(fresh, param, fj, 5, NWORD, 0.5)
    fresh.close()
    assert a == b and mid == ref and a != mid
