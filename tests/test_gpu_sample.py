"""GPU: sampled caption generation (lrcn_sample_batch, include/lrcn_sample.h) on all three routes of its per-step draw -- the Gumbel records
of the logits GEMM's epilogue (bf16, top_k 0), the top-K records (top_k < 6) and the row kernel on plain logits (f32, top_k >= 6,
LRCN_DECODE_SMAX=0) -- against beam search at width 1, a teacher-forced replay through the CPU oracle with the host restatement of the noise
(tests/philox_ref.py), a chi-squared test of the first-token distribution, and each other."""
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
import philox_ref as ph  # noqa: E402
import stage_boundary as sb  # noqa: E402

pytestmark = pytest.mark.gpu

E = H = 1000
V = 10640      # the production decode shape: 1024 images x 5 samples = 5120 rows
NP, SP, NWORD = 1024, 5, 8


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


def small_model(n_layers=2, seed=3, Vs=203, Es=64):
    m = orc.init_weights(Es, Es, Es, Vs, seed=seed, n_layers=n_layers)
    m.p["Wout"][:] *= 4.0   # a little spread in the word distributions, still far from peaky
    return m


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


_production = {}


def production():
    """One bf16 context + decisive model at the production shape, shared by the tests of this file (the context holds ~1 GB of tables)."""
    if not _production:
        m = decisive_model()
        ctx = L.Context(E, H, H, V, max_B=NP * SP, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        _production.update(m=m, ctx=ctx, param=L.model_from_arrays(m.p), feats=feats_of(NP, 11))
    return _production


def teardown_module(module):
    if _production:
        _production["ctx"].close()
        _production.clear()


def flat(res):
    return [row for img in res for row in img]


def replay(m, feats, res, S, T, top_k, seed, rows, bf16):
    """Teacher-forced replay of GPU samples `rows` (row r = image r // S, sample r % S) through the oracle: at every step the GPU's token
    must be an admitted column whose host score z / T + g is within delta of the host maximum, and the GPU's log-likelihood must be the host
    sum of log softmax(z)[token].  Returns (exact steps, steps)."""
    fl = flat(res)
    Tn = max(len(fl[r][0]) for r in rows) - 1
    toks = np.zeros((max(Tn, 1), len(rows)), np.int32)
    for b, r in enumerate(rows):
        seq = fl[r][0]
        for t in range(len(seq) - 2):   # inputs after bos: seq[1 .. len-2] (the last token is never fed)
            toks[t, b] = seq[t + 1]
    f = np.stack([feats[r // S] for r in rows])
    if bf16:
        with orc.emulate_bf16():
            z_all = orc.forward_logits(m, f, toks)
    else:
        z_all = orc.forward_logits(m, f, toks)
    exact = steps = 0
    for b, r in enumerate(rows):
        seq, lp = fl[r]
        i, s = r // S, r % S
        host_lp = 0.0
        for t in range(len(seq) - 1):
            z = z_all[t, b]
            tok = seq[t + 1]
            cols, sc = ph.scores(z, T, top_k, seed, i, s, t + 1)
            best = float(sc.max())
            # f32: the logits agree to ~1e-6 relative.  bf16: the emulating oracle rounds where the library rounds but sums in another
            # order, so an element of h can land one bf16 step (2^-8 relative) away; through |Wout| that moves a logit by up to ~1 %
            delta = (2e-2 if bf16 else 1e-4) * (1.0 + abs(best))
            assert tok in cols, ("token outside the admitted columns", r, t, tok)
            got = float(sc[list(cols).index(tok)])
            assert got >= best - delta, (r, t, tok, got, best)
            exact += int(cols[int(np.argmax(sc))] == tok)
            steps += 1
            host_lp += ph.log_softmax(z)[tok]
        tol = (5e-2 + 2e-2 * abs(host_lp)) if bf16 else (1e-3 + 1e-4 * abs(host_lp))
        assert abs(lp - host_lp) <= tol, (r, lp, host_lp)
    return exact, steps


# ------------------------------------------------------------------------------------------------ 1. greedy == beam search, K = 1
def test_greedy_equals_beam_width_1_f32_row_kernel():
    m = small_model()
    N = 12
    ctx = L.Context(64, 64, 64, 203, max_B=N, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 1))
    beam = L.beam_search_batch(ctx, param, fj, 1, NWORD)
    smp = L.sample_batch(ctx, param, fj, 1, NWORD, temperature=0.0, seed=123)
    for (bt, bp), img in zip(beam, smp):
        st, lp = img[0]
        assert st == bt
        if bp > 1e-30:
            assert abs(lp - np.log(bp)) <= 1e-4 * (1 + abs(lp)), (lp, np.log(bp))
    ctx.close()


def test_greedy_equals_beam_width_1_bf16_production_fused():
    P = production()
    N = NP * SP   # 5120 rows, one sample each
    feats = feats_of(N, 2)
    fj = L.to_jl(feats)
    beam = L.beam_search_batch(P["ctx"], P["param"], fj, 1, NWORD)
    smp = L.sample_batch(P["ctx"], P["param"], fj, 1, NWORD, temperature=0.0, seed=5)
    assert [t for t, _ in beam] == [img[0][0] for img in smp]
    for (bt, bp), img in zip(beam, smp):
        if bp > 1e-30:
            assert abs(img[0][1] - np.log(bp)) <= 2e-3 * (1 + abs(img[0][1])), (img[0][1], np.log(bp))


# ------------------------------------------------------------------------------------------------ 2. teacher-forced replay
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("T,top_k", [(1.0, 0), (0.7, 0), (1.0, 3), (0.7, 10)])
def test_replay_small_f32(n_layers, T, top_k):
    m = small_model(n_layers=n_layers)
    N, S, seed = 6, 4, 0x1234567890ABCDEF
    ctx = L.Context(64, 64, 64, 203, max_B=N * S, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)
    param = L.model_from_arrays(m.p)
    feats = feats_of(N, 7)
    res = L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, temperature=T, top_k=top_k, seed=seed)
    assert len(res) == N and all(len(img) == S for img in res)
    for img in res:
        for seq, _ in img:
            assert seq[0] == 1   # bos (0-based ids)
            assert 2 <= len(seq) <= NWORD + 2
            assert all(t != 0 for t in seq[1:-1])   # eos ends a caption
    exact, steps = replay(m, feats, res, S, T, top_k, seed, list(range(N * S)), bf16=False)
    assert exact == steps, (exact, steps)
    ctx.close()


@pytest.mark.parametrize("T,top_k", sb.DRAWS)
@pytest.mark.parametrize("V", sb.STAGE_V)
def test_replay_f32_at_the_stage_boundary(V, T, top_k):
    """k_sample_rows (the row-kernel route: an f32 context) at the last width whose logits row it stages in LDS and at the first it does
    not, on tests/stage_boundary.py's model: the last word holds a quarter of every row (tests/test_sample_host.py shows that the host's
    own sampler draws it).  Every step of every sample must be the host's argmax under the device's own prefix, and the device must have
    drawn the last word too.

    A local build (not kept) whose staged copy lost its last element (row_max_stage read it as -inf) failed both cases at V = 15360 (top_k
    0: a drawn word 1.5 below the host's best score; top_k 3: word 15343 drawn, the host's admitted columns 9993, 14720, 15359) and passed
    both at 15361."""
    m, feats = sb.model(V), sb.feats()
    ctx = L.Context(sb.E, sb.H, sb.H, V, max_B=sb.N * sb.S, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    res = L.sample_batch(ctx, L.model_from_arrays(m.p), L.to_jl(feats), sb.S, sb.NWORD, temperature=T, top_k=top_k, seed=sb.SEED)
    ctx.close()
    assert len(res) == sb.N and all(len(img) == sb.S for img in res)
    exact, steps = replay(m, feats, res, sb.S, T, top_k, sb.SEED, list(range(sb.N * sb.S)), bf16=False)
    assert exact == steps, (exact, steps)
    assert any(t == V - 1 for seq, _ in flat(res) for t in seq[1:])


@pytest.mark.parametrize("route", ["fused-gumbel", "fused-topk3", "row-kernel"])
def test_replay_production_bf16(route, monkeypatch):
    P = production()
    top_k = 3 if route == "fused-topk3" else 0
    monkeypatch.setenv("LRCN_DECODE_SMAX", "0" if route == "row-kernel" else "1")
    seed = 99
    res = L.sample_batch(P["ctx"], P["param"], L.to_jl(P["feats"]), SP, NWORD, temperature=1.0, top_k=top_k, seed=seed)
    R = NP * SP
    rows = sorted(set([0, 1, 2, 3, 4, 255, 256, 1279, 2560, 2561, 4095, R - 6, R - 2, R - 1] + list(range(7, R, 157))))
    exact, steps = replay(P["m"], P["feats"], res, SP, 1.0, top_k, seed, rows, bf16=True)
    print("route %s: %d of %d steps the exact host argmax" % (route, exact, steps))
    assert exact >= 0.99 * steps, (exact, steps)


# ------------------------------------------------------------------------------------------------ 3. distribution
@pytest.mark.parametrize("top_k,knob", [(0, "1"), (5, "1"), (0, "0")])
def test_first_token_distribution_chi2(top_k, knob, monkeypatch):
    from scipy.stats import chi2
    Ed, Vd, S = 256, 2048, 4096
    m = orc.init_weights(Ed, Ed, Ed, Vd, seed=21)
    m.p["bout"][:] = (np.random.default_rng(8).standard_normal((1, Vd)) * 2.5).astype(np.float32)   # a few hundred likely words
    ctx = L.Context(Ed, Ed, Ed, Vd, max_B=S, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.model_from_arrays(m.p)
    feat = feats_of(1, 9)
    monkeypatch.setenv("LRCN_DECODE_SMAX", knob)
    res = L.sample_batch(ctx, param, L.to_jl(feat), S, 1, temperature=1.0, top_k=top_k, seed=2024)[0]
    ctx.close()
    first = np.array([seq[1] for seq, _ in res])
    with orc.emulate_bf16():
        z = orc.forward_logits(m, feat, np.zeros((1, 1), np.int32))[0, 0].astype(np.float64)
    cols = ph.admitted(z.astype(np.float32), top_k)
    p = np.zeros(Vd)
    p[cols] = np.exp(z[cols] - z[cols].max())
    p /= p.sum()
    assert np.isin(first, cols).all()
    obs = np.bincount(first, minlength=Vd).astype(np.float64)
    exp_ = p * S
    big = exp_ >= 5
    o = np.append(obs[big], obs[~big].sum())
    e = np.append(exp_[big], exp_[~big].sum())
    keep = e > 0
    stat = float(((o[keep] - e[keep]) ** 2 / e[keep]).sum())
    dof = int(keep.sum()) - 1
    pval = chi2.sf(stat, dof)
    print("top_k %d, LRCN_DECODE_SMAX=%s: chi2 %.1f on %d dof, p = %.3g" % (top_k, knob, stat, dof, pval))
    assert dof >= 4
    assert pval > 1e-3, (stat, dof, pval)


# ------------------------------------------------------------------------------------------------ 4. routes agree
@pytest.mark.parametrize("top_k", [0, 3])
def test_fused_routes_agree_with_the_row_kernel(top_k, monkeypatch):
    P = production()
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("LRCN_DECODE_SMAX", knob)
        out[knob] = flat(L.sample_batch(P["ctx"], P["param"], L.to_jl(P["feats"]), SP, NWORD, temperature=1.0, top_k=top_k, seed=7))
    R = NP * SP
    same = sum(a[0] == b[0] for a, b in zip(out["1"], out["0"]))
    print("top_k %d: %d of %d rows identical" % (top_k, same, R))
    assert same >= R - R // 50, (same, R)
    for a, b in zip(out["1"], out["0"]):
        if a[0] == b[0]:
            assert abs(a[1] - b[1]) <= 5e-2 + 2e-2 * abs(b[1]), (a[1], b[1])


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_seed_repeats_and_changes_row_kernel():
    m = small_model()
    N, S = 8, 4
    ctx = L.Context(64, 64, 64, 203, max_B=N * S, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    feats = feats_of(N, 4)
    a = flat(L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, seed=1))
    b = flat(L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, seed=1))
    c = flat(L.sample_batch(ctx, param, L.to_jl(feats), S, NWORD, seed=2))
    assert a == b
    assert sum(x[0] != y[0] for x, y in zip(a, c)) >= 0.9 * N * S
    # image 3's samples do not depend on the other images of the call: bit-equal on this route
    f2 = feats_of(N, 5)
    f2[3] = feats[3]
    d = L.sample_batch(ctx, param, L.to_jl(f2), S, NWORD, seed=1)[3]
    assert d == a[3 * S:4 * S]
    ctx.close()


def test_seed_repeats_and_image_independence_fused():
    P = production()
    fj = L.to_jl(P["feats"])
    a = flat(L.sample_batch(P["ctx"], P["param"], fj, SP, NWORD, seed=3))
    b = flat(L.sample_batch(P["ctx"], P["param"], fj, SP, NWORD, seed=3))
    assert a == b
    f2 = feats_of(NP, 12)
    keep = np.arange(0, NP, 2)
    f2[keep] = P["feats"][keep]   # every other image the same, the rest replaced
    d = flat(L.sample_batch(P["ctx"], P["param"], L.to_jl(f2), SP, NWORD, seed=3))
    rows = [i * SP + s for i in keep for s in range(SP)]
    same = sum(a[r][0] == d[r][0] for r in rows)
    assert same >= len(rows) - len(rows) // 50, (same, len(rows))


def test_different_seed_changes_rows_fused():
    """At T = 1 on a flat model (the initial weights: no word dominates), another seed changes almost every row."""
    m = orc.init_weights(256, 256, 256, 2048, seed=1)
    N, S = 128, 4
    ctx = L.Context(256, 256, 256, 2048, max_B=N * S, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 6))
    a = flat(L.sample_batch(ctx, param, fj, S, NWORD, seed=10))
    c = flat(L.sample_batch(ctx, param, fj, S, NWORD, seed=11))
    ctx.close()
    assert sum(x[0] != y[0] for x, y in zip(a, c)) >= 0.9 * N * S


# ------------------------------------------------------------------------------------------------ 6. argument errors
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

    def call(N_, S, nword, T, k):
        return lib.lrcn_sample_batch(ctx._h, L._p9(param), L._ptr(fj), N_, S, nword, T, k, 1, out, n, lp)

    assert call(N, 2, 4, 1.0, 0) == 0
    bad = [(N, 0, 4, 1.0, 0), (N, 3, 4, 1.0, 0), (0, 1, 4, 1.0, 0),          # S < 1, N*S > max_B, N < 1
           (N, 1, 4, -0.5, 0), (N, 1, 4, float("nan"), 0), (N, 1, 4, float("inf"), 0),
           (N, 1, 4, 1.0, -1), (N, 1, 4, 1.0, 33),
           (N, 1, 0, 1.0, 0), (N, 1, 257, 1.0, 0)]
    for args in bad:
        assert call(*args) == -1, args   # LRCN_EINVAL
        assert lib.lrcn_last_error(ctx._h)
    ctx.close()
    tiny = L.Context(16, 16, 16, 20, max_B=4, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    mt = orc.init_weights(16, 16, 16, 20, seed=1)
    pt = L.model_from_arrays(mt.p)
    f1 = L.to_jl(feats_of(1, 1))
    assert lib.lrcn_sample_batch(tiny._h, L._p9(pt), L._ptr(f1), 1, 1, 4, 1.0, 21, 1, out, n, lp) == -1   # top_k > V
    assert lib.lrcn_sample_batch(tiny._h, L._p9(pt), L._ptr(f1), 1, 1, 4, 1.0, 20, 1, out, n, lp) == 0
    tiny.close()
