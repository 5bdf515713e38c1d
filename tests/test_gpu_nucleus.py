"""GPU: nucleus (top-p) sampling and top_k of any width (include/lrcn_nucleus.h).  The selection is proven exact through lrcn_sample_logits
on logits built on the host (tests/nucleus_ref.py: rows whose intended nucleus size is decisive by construction, natural rows inside a
derived band, ties at the boundary, wide top_k, the combination, a chi-squared test of the draw, log-probabilities, repeatability); then
lrcn_sample_batch_p: bit-equality with lrcn_sample_batch where it falls through, a teacher-forced replay through the CPU oracle, the
production shape in bf16, repeatability, image independence and argument errors."""
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
import nucleus_ref as nr  # noqa: E402
import philox_ref as ph  # noqa: E402

pytestmark = pytest.mark.gpu

NWORD = 8
_ctx = {}


def small_ctx():
    """One small f32 context for every lrcn_sample_logits call (the entry is independent of the model sizes)."""
    if not _ctx:
        _ctx["c"] = L.Context(16, 16, 16, 20, max_B=4, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    return _ctx["c"]


_production = {}


def teardown_module(module):
    if _ctx:
        _ctx.pop("c").close()
    if _production:
        _production["ctx"].close()
        _production.clear()


def check_logp(z_rows, tok, lp):
    """11: the reported log-probability is log softmax(z)[tok] over the WHOLE row at temperature 1 (the project's f32 figure)."""
    for r, z in enumerate(z_rows):
        ref = float(ph.log_softmax(z)[tok[r]])
        assert abs(float(lp[r]) - ref) <= 1e-3 + 1e-4 * abs(ref), (r, float(lp[r]), ref)


# ------------------------------------------------------------------------------------------------ 5. exact size on decisive rows
@pytest.mark.parametrize("T", nr.DECISIVE_T)
@pytest.mark.parametrize("V", nr.DECISIVE_V)
def test_exact_size_on_decisive_rows(V, T):
    """V = 15360 | 15361 sit on both sides of the `stage` flag (the row kept in LDS up to 15360 columns); their rows carry the largest share
    in column V - 1 (nucleus_ref.STAGE_BOUNDARY_V).  A local build (not kept) whose staged copy lost its last element (row_max_stage read
    it as -inf) failed [15360-1.0] and [15360-0.7] on the n* = 1 row's draw (10953 and 3991 for the host's 15359), [37-*] and [203-*] on
    the log-probability (2e-3 .. 2.7e-2 > 1.3e-3), and passed [10640-*], where the last column holds 1e-4 of the row, and the unstaged
    15361 and 16411."""
    ctx, S = small_ctx(), nr.DECISIVE_S
    host = nr.decisive_host_draws(V, T)
    excused = 0
    for (z, top_p, n_star), (htok, hexc) in zip(nr.decisive_cases(V, T), host):
        rows = np.stack([z] * S)
        tok, lp, cnt = L.sample_logits(ctx, rows, S, 1, T, 0, top_p, nr.DECISIVE_SEED)
        print("V %d T %.1f n* %d top_p %.4f: counts %s" % (V, T, n_star, top_p, cnt.tolist()))
        assert (cnt == n_star).all(), (V, T, n_star, cnt.tolist())
        for s in range(S):
            if hexc[s]:
                excused += 1
                assert tok[s] in nr.admitted(z, T, 0, top_p)
            else:
                assert tok[s] == htok[s], (V, T, n_star, s, int(tok[s]), int(htok[s]))
        check_logp(rows, tok, lp)
    print("V %d T %.1f: %d draws excused" % (V, T, excused))


# ------------------------------------------------------------------------------------------------ 6. natural rows, any n
BAND = 2e-3   # an f32 sum of V <= 16411 non-negative terms in any order is within (V - 1) 2^-24 < 1e-3 relative of the true sum; prefix and
#               total are both such sums, and an f32 exp on [-88, 0] adds well under 1e-4


@pytest.mark.parametrize("V", [10640, 16411])
def test_size_on_natural_rows(V):
    ctx, S, seed = small_ctx(), 2, 0xABCDEF0123
    base = nr.natural_rows(V, V)
    rows = np.repeat(base, S, axis=0)
    sizes = []
    for T in (0.7, 1.0, 1.5):
        Gs = [nr.nucleus_size(z, T, 0, 1.0)[1] for z in base]
        for top_p in (0.5, 0.9, 0.99):
            tok, lp, cnt = L.sample_logits(ctx, rows, S, 3, T, 0, top_p, seed)
            for r in range(rows.shape[0]):
                G, n = Gs[r // S], int(cnt[r])
                print("V %d T %.1f top_p %.2f row %d: n_dev %d (host %d), G[n] %.6f G[n-1] %.6f"
                      % (V, T, top_p, r, n, nr.nucleus_size(rows[r], T, 0, top_p)[0], G[min(n, V)], G[max(n - 1, 0)]))
                assert 1 <= n <= V
                assert G[n] >= top_p - BAND and G[n - 1] < top_p + BAND, (V, T, top_p, r, n, G[n], G[n - 1])
                sizes.append(n)
            assert (cnt.reshape(-1, S) == cnt.reshape(-1, S)[:, :1]).all()   # the size does not depend on the sample
            htok, hexc = nr.check_draws(rows, S, T, 0, top_p, seed, 3, counts=cnt)
            for r in range(rows.shape[0]):
                assert tok[r] in nr.rank_order(rows[r])[:cnt[r]]
                assert hexc[r] or tok[r] == htok[r], (V, T, top_p, r, int(tok[r]), int(htok[r]))
            check_logp(rows, tok, lp)
    assert min(sizes) <= 10 and max(sizes) >= 1000, (min(sizes), max(sizes))


# ------------------------------------------------------------------------------------------------ 7. ties at the boundary
@pytest.mark.parametrize("V", [203, 10640, 16411])
def test_ties_at_the_boundary(V):
    ctx, S = small_ctx(), 256
    rng = np.random.default_rng([V, 7])
    z, top_p, n_star, tcols = nr.tie_row_top_p(V, 1.0, rng)
    zk, top_k, kcols = nr.tie_row_top_k(V, 1.0, rng)
    for z_, k_, p_, n_, seed0 in ((z, 0, top_p, n_star, 100), (zk, top_k, 1.0, top_k, 200)):
        rows = np.stack([z_] * S)
        for seed in range(seed0, seed0 + 50):   # a seed whose 256 host draws hold no near-tie: then every token is decided
            htok, hexc = nr.check_draws(rows, S, 1.0, k_, p_, seed, 2)
            if not hexc.any():
                break
        assert not hexc.any()
        tok, lp, cnt = L.sample_logits(ctx, rows, S, 2, 1.0, k_, p_, seed)
        assert (cnt == n_).all(), (V, k_, cnt[:8].tolist(), n_)
        assert (tok == htok).all(), (V, k_, np.flatnonzero(tok != htok)[:8].tolist())
        check_logp(rows, tok, lp)
    # the draws reach the admitted tied columns (the lower ones) and no other tied column
    tok, _, _ = L.sample_logits(ctx, np.stack([z] * S), S, 2, 1.0, 0, top_p, 100)
    assert set(tok.tolist()) & set(tcols.tolist()) <= set(tcols[:3].tolist())


# ------------------------------------------------------------------------------------------------ 8. top_k above 32
@pytest.mark.parametrize("V", [10640, 16411])
def test_top_k_above_32(V):
    ctx, S, T = small_ctx(), 2, 1.0
    rows = np.repeat(nr.natural_rows(V, V + 1, per_std=2), S, axis=0)
    for top_k in (33, 100, 1000, V):
        for seed in range(300, 350):
            hs = [ph.scores(z, T, top_k, seed, r // S, r % S, 1) for r, z in enumerate(rows)]
            if not any(nr.excused(sc) for _, sc in hs):
                break
        htok = np.array([int(cols[np.argmax(sc)]) for cols, sc in hs])
        assert not any(nr.excused(sc) for _, sc in hs)
        tok, lp, cnt = L.sample_logits(ctx, rows, S, 1, T, top_k, 1.0, seed)
        assert (cnt == top_k).all(), (top_k, cnt.tolist())
        assert (tok == htok).all(), (top_k, tok.tolist(), htok.tolist())
        check_logp(rows, tok, lp)
        if top_k == V:
            tok0, lp0, cnt0 = L.sample_logits(ctx, rows, S, 1, T, 0, 1.0, seed)
            assert (tok0 == tok).all() and lp0.tobytes() == lp.tobytes() and (cnt0 == V).all()


# ------------------------------------------------------------------------------------------------ 9. combination
@pytest.mark.parametrize("V", [203, 10640])
def test_top_k_50_with_top_p(V):
    ctx, S, T, seed = small_ctx(), 4, 0.7, 77
    rng = np.random.default_rng([V, 9])
    for n_star in nr.COMBO_N:
        z, _ = nr.combo_row(V, T, n_star, rng)
        rows = np.stack([z] * S)
        tok, lp, cnt = L.sample_logits(ctx, rows, S, 1, T, 50, 0.9, seed)
        assert (cnt == n_star).all(), (V, n_star, cnt.tolist())
        htok, hexc = nr.check_draws(rows, S, T, 50, 0.9, seed, 1)
        assert all(hexc[r] or tok[r] == htok[r] for r in range(S)), (tok.tolist(), htok.tolist())
        check_logp(rows, tok, lp)


# ------------------------------------------------------------------------------------------------ 10. distribution
def test_nucleus_draw_distribution_chi2():
    from scipy.stats import chi2
    ctx, Vd, S, calls = small_ctx(), 2048, 256, 16   # 4096 draws of one row, 256 rows per call at step current = 1 .. 16
    z = (np.random.default_rng(8).standard_normal(Vd) * 2.5).astype(np.float32)
    rows = np.stack([z] * S)
    toks, cnts = [], []
    for call in range(calls):
        tok, _, cnt = L.sample_logits(ctx, rows, S, 1 + call, 1.0, 0, 0.9, 2024)
        toks.append(tok)
        cnts.append(cnt)
    first, cnt = np.concatenate(toks), np.concatenate(cnts)
    assert (cnt == cnt[0]).all()
    n = int(cnt[0])
    G = nr.nucleus_size(z, 1.0, 0, 1.0)[1]
    assert G[n] >= 0.9 - BAND and G[n - 1] < 0.9 + BAND
    cols = nr.admitted(z, 1.0, 0, 0.9, n=n)   # the device's own nucleus
    z64 = z.astype(np.float64)
    p = np.zeros(Vd)
    p[cols] = np.exp(z64[cols] - z64[cols].max())
    p /= p.sum()
    assert np.isin(first, cols).all()
    obs = np.bincount(first, minlength=Vd).astype(np.float64)
    exp_ = p * first.shape[0]
    big = exp_ >= 5
    o = np.append(obs[big], obs[~big].sum())
    e = np.append(exp_[big], exp_[~big].sum())
    keep = e > 0
    stat = float(((o[keep] - e[keep]) ** 2 / e[keep]).sum())
    dof = int(keep.sum()) - 1
    pval = chi2.sf(stat, dof)
    print("nucleus of %d columns: chi2 %.1f on %d dof, p = %.3g" % (n, stat, dof, pval))
    assert dof >= 4
    assert pval > 1e-3, (stat, dof, pval)


# ------------------------------------------------------------------------------------------------ 12. repeatability
def test_logits_entry_repeats_and_seed_changes():
    ctx, V, R, S = small_ctx(), 10640, 256, 4
    rows = (0.1 * np.random.default_rng(3).standard_normal((R, V))).astype(np.float32)   # flat: no word dominates
    a = L.sample_logits(ctx, rows, S, 1, 1.0, 0, 0.9, 1)
    b = L.sample_logits(ctx, rows, S, 1, 1.0, 0, 0.9, 1)
    c = L.sample_logits(ctx, rows, S, 1, 1.0, 0, 0.9, 2)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[0] != c[0]).sum() >= 0.9 * R
    assert (a[2] == c[2]).all()   # the nucleus does not depend on the seed
    check_logp(rows[:16], a[0][:16], a[1][:16])
    # greedy: top_k and top_p have no effect
    g = L.sample_logits(ctx, rows[:8], S, 1, 0.0, 5, 0.3, 1)
    assert (g[0] == rows[:8].argmax(axis=1)).all() and (g[2] == V).all()


# ================================================================================================ lrcn_sample_batch_p
def small_model(n_layers=2, seed=3, Vs=203, Es=64):
    m = orc.init_weights(Es, Es, Es, Vs, seed=seed, n_layers=n_layers)
    m.p["Wout"][:] *= 4.0   # a little spread in the word distributions, still far from peaky
    return m


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


def production():
    """One bf16 context + model at the production shape (E = H = 1000, V = 10640, 1024 x 5 rows), shared by the tests of this file."""
    if not _production:
        m = nr.production_model()
        ctx = L.Context(nr.PROD_E, nr.PROD_H, nr.PROD_H, nr.PROD_V, max_B=nr.PROD_N * nr.PROD_S, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        _production.update(m=m, ctx=ctx, param=L.model_from_arrays(m.p), feats=nr.production_feats())
    return _production


def flat(res):
    return [row for img in res for row in img]


# ------------------------------------------------------------------------------------------------ 13. falls through to today's sampler
@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("top_k", [0, 3, 10])
def test_top_p_1_is_todays_sampler_small_f32(top_k, knob, monkeypatch):
    monkeypatch.setenv("LRCN_DECODE_SMAX", knob)
    m = small_model()
    N, S = 12, 4
    ctx = L.Context(64, 64, 64, 203, max_B=N * S, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param, fj = L.model_from_arrays(m.p), L.to_jl(feats_of(N, 7))
    old = L.sample_batch(ctx, param, fj, S, NWORD, temperature=0.9, top_k=top_k, seed=41)
    new, cnt = L.sample_batch(ctx, param, fj, S, NWORD, temperature=0.9, top_k=top_k, seed=41, top_p=1.0, return_counts=True)
    ctx.close()
    assert new == old   # tokens, lengths and log-probabilities, bit for bit
    for r, (seq, _) in enumerate(flat(new)):
        steps = len(seq) - 1
        assert (cnt.reshape(N * S, -1)[r, :steps] == (top_k or 203)).all() and (cnt.reshape(N * S, -1)[r, steps:] == 0).all()


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("top_k", [0, 3, 10])
def test_top_p_1_is_todays_sampler_production_bf16(top_k, knob, monkeypatch):
    monkeypatch.setenv("LRCN_DECODE_SMAX", knob)
    P = production()
    fj = L.to_jl(P["feats"])
    old = L.sample_batch(P["ctx"], P["param"], fj, nr.PROD_S, NWORD, temperature=1.0, top_k=top_k, seed=17)
    new = L.sample_batch(P["ctx"], P["param"], fj, nr.PROD_S, NWORD, temperature=1.0, top_k=top_k, seed=17, top_p=1.0, return_counts=True)[0]
    assert new == old


# ------------------------------------------------------------------------------------------------ 14. teacher-forced replay, f32
def replay_nucleus(m, feats, res, counts, S, T, top_k, top_p, seed, rows):
    """Teacher-forced replay through the oracle.  With the oracle's logits z and the band b = 2e-3 + (exp(2 dz / T) - 1), dz = 1e-4 (1 +
    max|z|) (the f32 logit agreement, through which any ratio of two weights can move): the token lies among the columns whose share BEFORE
    them is < top_p + b, its score is at least the best score over the columns whose share THROUGH them is < top_p - b (minus the delta of
    test_gpu_sample.replay); the first-ranked column counts as admitted in both sets; the count satisfies the two-sided condition with b."""
    fl = flat(res)
    Tn = max(len(fl[r][0]) for r in rows) - 1
    toks = np.zeros((max(Tn, 1), len(rows)), np.int32)
    for b_, r in enumerate(rows):
        seq = fl[r][0]
        for t in range(len(seq) - 2):
            toks[t, b_] = seq[t + 1]
    z_all = orc.forward_logits(m, np.stack([feats[r // S] for r in rows]), toks)
    steps = 0
    for b_, r in enumerate(rows):
        seq, lp = fl[r]
        host_lp = 0.0
        for t in range(len(seq) - 1):
            z, tok, n_dev = z_all[t, b_], seq[t + 1], int(counts[r, t])
            band = BAND + float(np.expm1(2.0 * 1e-4 * (1.0 + np.abs(z).max()) / T))
            order = nr.rank_order(z)
            G = nr.nucleus_size(z, T, top_k, 1.0)[1]          # G[m]: share of the first m columns of A_k
            k = G.shape[0] - 1
            wide = G[:k] < top_p + band                       # rank m's share before it
            narrow = G[1:] < top_p - band                     # rank m's share through it
            wide[0] = narrow[0] = True
            wcols, ncols = order[:k][wide], order[:k][narrow]
            assert tok in wcols, ("token outside the widest admissible nucleus", r, t, tok)
            g = ph.noise(seed, r // S, r % S, t + 1, np.arange(z.shape[0]))
            sc = z.astype(np.float32) / np.float32(T) + g
            best = float(sc[ncols].max())
            assert float(sc[tok]) >= best - 1e-4 * (1.0 + abs(best)), (r, t, tok, float(sc[tok]), best)
            assert 1 <= n_dev <= k and G[n_dev] >= top_p - band and G[n_dev - 1] < top_p + band, (r, t, n_dev, G[n_dev], G[n_dev - 1], band)
            host_lp += ph.log_softmax(z)[tok]
            steps += 1
        assert (counts[r, len(seq) - 1:] == 0).all()
        assert abs(lp - host_lp) <= 1e-3 + 1e-4 * abs(host_lp), (r, lp, host_lp)
    return steps


@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 0.9), (0.7, 0, 0.5), (1.0, 50, 0.9)])
def test_replay_small_f32(n_layers, T, top_k, top_p):
    m = small_model(n_layers=n_layers)
    N, S, seed = 6, 4, 0x1234567890ABCDEF
    ctx = L.Context(64, 64, 64, 203, max_B=N * S, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)
    feats = feats_of(N, 7)
    res, cnt = L.sample_batch(ctx, L.model_from_arrays(m.p), L.to_jl(feats), S, NWORD, temperature=T, top_k=top_k, seed=seed, top_p=top_p,
                              return_counts=True)
    ctx.close()
    for seq, _ in flat(res):
        assert seq[0] == 1 and 2 <= len(seq) <= NWORD + 2 and all(t != 0 for t in seq[1:-1])
    cnt = cnt.reshape(N * S, NWORD + 1)
    steps = replay_nucleus(m, feats, res, cnt, S, T, top_k, top_p, seed, list(range(N * S)))
    print("n_layers %d T %.1f top_k %d top_p %.2f: %d steps, nucleus sizes %d .. %d" % (n_layers, T, top_k, top_p, steps, cnt[cnt > 0].min(), cnt.max()))
    assert cnt[cnt > 0].min() < (top_k or 203)   # the nucleus did cut


# ------------------------------------------------------------------------------------------------ 15. production shape, bf16
def test_tight_nucleus_is_greedy_production_bf16(monkeypatch):
    """Through bf16 logits the band of the replay is too wide to bind, so the check is structural: at top_p = 0.05 a row whose top word holds
    >= 10 % at every step (by the bf16-emulating oracle: a JUDGED row) has the nucleus {top word} and must give the greedy caption.  Both
    calls read the plain f32 logits (LRCN_DECODE_SMAX=0 for the greedy one: the route every nucleus call takes), so they see the same bits."""
    monkeypatch.setenv("LRCN_DECODE_SMAX", "0")
    P = production()
    fj, S = L.to_jl(P["feats"]), nr.PROD_S
    greedy = flat(L.sample_batch(P["ctx"], P["param"], fj, S, NWORD, temperature=0.0, seed=5))
    tight, cnt = L.sample_batch(P["ctx"], P["param"], fj, S, NWORD, temperature=1.0, top_k=0, seed=5, top_p=0.05, return_counts=True)
    tight, cnt = flat(tight), cnt.reshape(nr.PROD_N * S, NWORD + 1)
    rows = nr.production_rows()
    jd = nr.judged(P["m"], np.stack([P["feats"][r // S] for r in rows]), [greedy[r][0] for r in rows])
    print("%d of %d sampled rows judged" % (int(jd.sum()), len(rows)))
    assert jd.sum() >= 0.5 * len(rows)
    for r, ok in zip(rows, jd):
        if ok:
            assert tight[r][0] == greedy[r][0], (r, tight[r][0], greedy[r][0])
            assert abs(tight[r][1] - greedy[r][1]) <= 5e-2 + 2e-2 * abs(greedy[r][1])
            assert (cnt[r, :len(tight[r][0]) - 1] == 1).all(), (r, cnt[r].tolist())


# ------------------------------------------------------------------------------------------------ 16. repeatability, image independence
def test_batch_repeats_and_image_independence():
    m = small_model()
    N, S = 8, 4
    ctx = L.Context(64, 64, 64, 203, max_B=N * S, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param, feats = L.model_from_arrays(m.p), feats_of(N, 4)
    a, ca = L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, seed=1, top_p=0.9, return_counts=True)
    b, cb = L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, seed=1, top_p=0.9, return_counts=True)
    assert a == b and ca.tobytes() == cb.tobytes()
    f2 = feats_of(N, 5)
    f2[3] = feats[3]
    d, cd = L.sample_batch(ctx, param, L.to_jl(f2), S, NWORD, seed=1, top_p=0.9, return_counts=True)
    assert d[3] == a[3] and cd[3].tobytes() == ca[3].tobytes()   # image 3's samples do not depend on the other images: bit-equal on f32
    assert L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, seed=1, top_p=0.9) == a
    ctx.close()


def test_batch_repeats_production_bf16():
    P = production()
    fj = L.to_jl(P["feats"])
    a, ca = L.sample_batch(P["ctx"], P["param"], fj, nr.PROD_S, NWORD, seed=3, top_p=0.9, return_counts=True)
    b, cb = L.sample_batch(P["ctx"], P["param"], fj, nr.PROD_S, NWORD, seed=3, top_p=0.9, return_counts=True)
    assert a == b and ca.tobytes() == cb.tobytes()
    k100, ck = L.sample_batch(P["ctx"], P["param"], fj, nr.PROD_S, NWORD, seed=3, top_k=100, return_counts=True)
    assert set(np.unique(ck).tolist()) <= {0, 100}


# ------------------------------------------------------------------------------------------------ 17. argument errors
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
    cnt = (C.c_int32 * (N * 8 * 300))()

    def call(N_, S, nword, T, k, p):
        return lib.lrcn_sample_batch_p(ctx._h, L._p9(param), L._ptr(fj), N_, S, nword, T, k, p, 1, out, n, lp, cnt)

    def launches():   # the rows' done counter is reset by every call that reaches the GPU; a refused call leaves the last result in place
        return bytes(out), bytes(cnt)

    assert call(N, 2, 4, 1.0, 0, 0.9) == 0
    assert call(N, 2, 4, 1.0, 33, 1.0) == 0          # top_k = 33 succeeds here
    assert call(N, 2, 4, 1.0, 203, 0.5) == 0
    before = launches()
    bad = [(N, 1, 4, 1.0, 0, 0.0), (N, 1, 4, 1.0, 0, -0.1), (N, 1, 4, 1.0, 0, 1.5), (N, 1, 4, 1.0, 0, float("nan")),
           (N, 1, 4, 1.0, -1, 0.9), (N, 1, 4, 1.0, 204, 0.9),
           (N, 0, 4, 1.0, 0, 0.9), (N, 3, 4, 1.0, 0, 0.9), (0, 1, 4, 1.0, 0, 0.9),
           (N, 1, 4, -0.5, 0, 0.9), (N, 1, 4, float("nan"), 0, 0.9), (N, 1, 4, float("inf"), 0, 0.9),
           (N, 1, 0, 1.0, 0, 0.9), (N, 1, 257, 1.0, 0, 0.9)]
    for args in bad:
        assert call(*args) == -1, args   # LRCN_EINVAL
        assert lib.lrcn_last_error(ctx._h)
        assert launches() == before      # nothing ran: the outputs of the last good call are untouched
    # the logits entry
    z = L.torch.zeros((2, 20), dtype=L.torch.float32, device="cuda:%d" % ctx.device)
    tok = L.torch.zeros(2, dtype=L.torch.int32, device=z.device)

    def lcall(ld, R, V, S, T, k, p):
        return lib.lrcn_sample_logits(ctx._h, C.c_void_p(z.data_ptr()), ld, R, V, S, 1, T, k, p, 1, C.c_void_p(tok.data_ptr()), None, None)

    assert lcall(20, 2, 20, 1, 1.0, 0, 0.9) == 0
    for args in [(19, 2, 20, 1, 1.0, 0, 0.9), (20, 0, 20, 1, 1.0, 0, 0.9), (20, 2, 0, 1, 1.0, 0, 0.9), (20, 2, 20, 0, 1.0, 0, 0.9),
                 (20, 2, 20, 1, -1.0, 0, 0.9), (20, 2, 20, 1, 1.0, 21, 0.9), (20, 2, 20, 1, 1.0, -1, 0.9), (20, 2, 20, 1, 1.0, 0, 0.0),
                 (20, 2, 20, 1, 1.0, 0, 1.01), (20, 2, 20, 1, 1.0, 0, float("nan"))]:
        assert lcall(*args) == -1, args
    ctx.sync()
    ctx.close()


# ================================================================================================ command line
def test_cli_generate_with_topp(tmp_path, capsys):
    """tools/lrcn.py --generate 20 --sample 5 --topp 0.9 writes candidates (the fixture of tests/test_gpu_sample_cli.py)."""
    import importlib
    import json
    from lrcn_amd import formats as fmt
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(48):
        a, b = img % 4, (img // 4) % 3
        f = np.zeros(4096, np.float32)
        f[a * 100:a * 100 + 50] = 1.0
        f[1000 + b * 100:1000 + b * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns.append({"image_id": img, "caption": "A %s %s ." % (nouns[a], verbs[b])})
    tr = str(tmp_path / "captions.json")
    with open(tr, "w") as fh:
        json.dump({"annotations": anns}, fh)
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)
    ck = str(tmp_path / "m.npz")
    common = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "8",
              "--atype", "f32", "--seed", "3"]
    assert cli.main(common + ["--train", "--epochs", "1", "--lr", "0.01", "--savefile", ck, "--dropout", "0.0"]) == 0
    capsys.readouterr()

    def run(name, extra):
        out = str(tmp_path / name)
        assert cli.main(common + ["--loadfile", ck, "--generate", "20", "--capnumber", "12", "--out", out, "--sample", "5"] + extra) == 0
        return [open(os.path.join(out, f)).read().splitlines() for f in ("candidates.txt", "candidate_ids.txt", "samples.txt")]

    p9 = run("p9", ["--topp", "0.9"])
    assert len(p9[0]) == len(p9[1]) == 12 and len(p9[2]) == 60 and all(c.endswith(".") for c in p9[0])
    assert run("p9b", ["--topp", "0.9"]) == p9                       # --seed fixes the draws
    assert run("p1", ["--topp", "1.0"]) == run("plain", [])          # the default is today's sampler
    tight = run("tight", ["--topp", "0.9", "--topk", "2"])
    assert len(tight[2]) == 60
