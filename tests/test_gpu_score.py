"""GPU: caption scoring (lrcn_score_matrix / lrcn_score_pairs, include/lrcn_score.h) -- s(n, m) = sum of log softmax(z_t)[y_t] over the
caption's words and eos -- against the CPU oracle's teacher-forced logits (f32 exactly, bf16 through the emulating oracle), across its routes
(the GEMM_OUT_SMAX_PICK epilogue against plain logits + k_softmax_xent), pieces, permutations, the sampler's log-likelihoods, and with the
beam decode on the same context."""
import ctypes as C

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L
from oracle import oracle as orc

import score_blocks_case as sc

pytestmark = pytest.mark.gpu

E = H = 1000
V = 10640      # the production decode shape: 64 images x 80 captions = 5120 pair rows
NP, MP = 64, 80


def decisive_model(seed=4):
    """As in test_gpu_sample.py: random weights scaled until the word distributions are peaky."""
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed)
    for n in ("W1", "W2", "Wout"):
        m.p[n] *= 2.0
    m.p["Wout"][:] *= 8.0
    m.p["bout"][:] = (rng.standard_normal((1, V)) * 2.0).astype(np.float32)
    m.p["b1"][:] += (rng.standard_normal(m.p["b1"].shape) * 0.5).astype(np.float32)
    return m


def small_model(seed=3, Vs=203, Es=64, n_layers=2):
    m = orc.init_weights(Es, Es, Es, Vs, seed=seed, n_layers=n_layers)
    m.p["Wout"][:] *= 4.0
    return m


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


def captions_of(M, Vs, seed, lens=None):
    """M captions of random words (ids 3 .. Vs-1: no eos / bos / unk inside), lengths `lens` or 1 .. 28."""
    rng = np.random.default_rng(seed)
    if lens is None:
        lens = rng.integers(1, 29, size=M)
    return [list(rng.integers(3, Vs, size=int(n))) for n in lens]


def oracle_scores(m, feats, caps, pairs, bf16=False):
    """s(n, m) for the (n, m) of `pairs` through orc.forward_logits, grouped by caption length."""
    out = {}
    by_len = {}
    for n, c in pairs:
        by_len.setdefault(len(caps[c]), []).append((n, c))
    for Lc, group in by_len.items():
        toks = np.array([caps[c] for _, c in group], np.int32).T.reshape(Lc, len(group))
        f = np.stack([feats[n] for n, _ in group])
        if bf16:
            with orc.emulate_bf16():
                z = orc.forward_logits(m, f, toks)
        else:
            z = orc.forward_logits(m, f, toks)
        z = z.astype(np.float64)
        lse = z.max(axis=2, keepdims=True) + np.log(np.exp(z - z.max(axis=2, keepdims=True)).sum(axis=2, keepdims=True))
        lp = z - lse
        for b, (n, c) in enumerate(group):
            y = list(caps[c]) + [0]
            out[(n, c)] = float(sum(lp[t, b, y[t]] for t in range(Lc + 1)))
    return out


_production = {}


def production():
    """One bf16 context + decisive model at the production shape, shared by the tests of this file."""
    if not _production:
        m = decisive_model()
        ctx = L.Context(E, H, H, V, max_B=NP * MP, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        rng = np.random.default_rng(21)
        lens = np.concatenate([[1, 28, 28, 1], rng.integers(1, 29, size=MP - 4)])
        rng.shuffle(lens)
        _production.update(m=m, ctx=ctx, param=L.model_from_arrays(m.p), feats=feats_of(NP, 11),
                           caps=captions_of(MP, V, 22, lens))
    return _production


def teardown_module(module):
    for d in (_production, _ride):
        if d:
            d["ctx"].close()
            d.clear()


def step_counts(caps):
    return np.array([len(c) + 1 for c in caps], np.float64)


# ------------------------------------------------------------------------------------------------ 1. f32 against the oracle
def test_f32_matrix_matches_oracle():
    m = small_model()
    N, M = 7, 23
    lens = np.array([5, 1, 28, 3, 12, 28, 7, 1, 9, 15, 2, 20, 4, 6, 11, 27, 8, 13, 3, 19, 1, 10, 22])
    caps = captions_of(M, 203, 5, lens)
    feats = feats_of(N, 1)
    ctx = L.Context(64, 64, 64, 203, max_B=64, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    s = L.score_matrix(ctx, param, L.to_jl(feats), caps)
    ctx.close()
    assert s.shape == (N, M)
    ref = oracle_scores(m, feats, caps, [(n, c) for n in range(N) for c in range(M)])
    for (n, c), v in ref.items():
        assert abs(s[n, c] - v) <= 1e-5 * (1 + abs(v)), (n, c, s[n, c], v)
    # the same through lrcn_loss with one row: s = -(L + 1) * loss
    lc = -(len(caps[2]) + 1) * orc.loss(m, feats[3:4], np.array(caps[2], np.int32).reshape(-1, 1))
    assert abs(s[3, 2] - lc) <= 1e-5 * (1 + abs(lc))


# ------------------------------------------------------------------------------------------------ 1b. every block loop more than once
def test_f32_every_block_loop_runs_more_than_once_vs_oracle():
    """score_impl cuts captions and images into blocks of max_B and pair rows into pieces of max_B.  max_B = 8 with 19 images (blocks of 8,
    8, 3) and 21 captions (8, 8, 5): the second and third iterations of the caption loop (`off[t] + j0` into the step inputs and into P_t)
    and of the image loop (`U2 + n0 * 4 * H2`, `feats + n0`), 50 pieces of the matrix and 5 of the pairs.  Every one of the 399 pairs against
    the oracle, test_f32_matrix_matches_oracle's bound; 37 pairs through score_pairs, the corners among them.

    A local build (not kept) whose caption loop read `d_in + off[t]` without `+ j0` failed here at the first pair of a caption outside
    block 0 (image 0, caption 12: -26.56923 against -26.57141, 2.2e-3 > 2.8e-4); every score test before this one passed it."""
    m = small_model()
    N, M = 19, 21
    lens = np.array([4, 1, 9, 3, 7, 9, 2, 1, 5, 6, 3, 8, 4, 2, 7, 1, 5, 9, 6, 3, 8])
    assert len(lens) == M and lens.min() == 1 and lens.max() == 9 and len(set(lens.tolist())) < M
    caps = captions_of(M, 203, 15, lens)
    feats = feats_of(N, 16)
    ctx = L.Context(64, 64, 64, 203, max_B=8, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats)
    s = L.score_matrix(ctx, param, fj, caps)
    rng = np.random.default_rng(17)
    pi, pc = rng.integers(0, N, size=37), rng.integers(0, M, size=37)
    pi[:4], pc[:4] = [0, N - 1, 5, 11], [M - 1, 0, 0, M - 1]
    assert {0, N - 1} <= set(pi.tolist()) and {0, M - 1} <= set(pc.tolist())
    sp = L.score_pairs(ctx, param, fj, caps, pi, pc)
    ctx.close()
    assert s.shape == (N, M) and sp.shape == (37,)
    ref = oracle_scores(m, feats, caps, [(n, c) for n in range(N) for c in range(M)])
    assert len(ref) == 399
    gap = max(abs(s[n, c] - v) / (1 + abs(v)) for (n, c), v in ref.items())
    print("f32, max_B 8: 399 pairs, max |gap| / (1 + |s|) = %.3g" % gap)
    for (n, c), v in ref.items():
        assert abs(s[n, c] - v) <= 1e-5 * (1 + abs(v)), (n, c, s[n, c], v)
    for q, (n, c) in enumerate(zip(pi.tolist(), pc.tolist())):
        v = ref[(n, c)]
        assert abs(sp[q] - v) <= 1e-5 * (1 + abs(v)), (q, n, c, sp[q], v)


# ------------------------------------------------------------------------------------------------ 1c. bf16: the caption-side cell epilogue
RA_LONG, RA_SHORT, RA_N, RA_P = sc.N_LONG, len(sc.SHORT_LENS), sc.N, sc.P   # 40, 260, 260, 520
_ride = {}


def ride_along():
    """tests/score_blocks_case.py -- edge68 at V = 300 (H = 68, every route predicate accepts), a model in which the fed word matters -- on
    a bf16 context of max_B = 256; 300 captions, 40 of length 6 and 260 of lengths 1 .. 5; 260 images; 520 pairs in which every caption
    and every image occurs.  score_impl then runs (tests/test_score_blocks_case.py restates the plan on the CPU)
      caption block 0   256 captions (the 40 long ones first) through decode_gates_epi with the token table gathered by `gx_idx = tok`:
                        256, then fewer active rows, 40 at the last step -- up to 216 rows ride along, reading indices past the step's own
      caption block 1   44 captions of one and two words: table gather + GEMM + cell kernel
      image blocks      256 and 4
      pieces            256 and 256 pair rows (cell epilogue + record epilogue, shrinking below 256 active rows) and 8 (GEMM + cell kernel,
                        f32 logits + k_softmax_xent)
    Returns the shared context and inputs (and, once the first test has run, its scores)."""
    if not _ride:
        c, m = sc.case(), sc.model()
        ctx = L.Context(m.E, m.H1, m.H2, sc.V, max_B=sc.MAX_B, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16, n_layers=m.n_layers)
        _ride.update(m=m, ctx=ctx, param=L.model_from_arrays(m.p), feats=c.feats, caps=c.caps, pi=c.pi, pc=c.pc, H=m.H1, V=sc.V)
    return _ride


def trace_lines(err):
    """[(M, N, K)] of LRCN_TRACE_ROUTES' lines: the contractions that went through the router (the cell-epilogue and record-epilogue GEMMs
    are launched directly and print nothing)."""
    out = []
    for line in err.splitlines():
        if line.startswith("gemm M="):
            f = line.split()
            out.append(tuple(int(x.split("=")[1]) for x in f[1:4]))
    return out


def test_bf16_caption_side_epilogue_with_ride_along_rows_vs_emulating_oracle(monkeypatch, capfd):
    """The call of ride_along() against the bf16-emulating oracle, all 520 pairs, test_bf16_production_matches_emulating_oracle's bound.

    The route: lrcn_debug_route names the call's last contraction only, and LRCN_TRACE_ROUTES prints the routed GEMMs, not the two epilogue
    launches.  So the trace shows the routes by what is absent: a gate GEMM (N = 4 H = 272) of 256 rows besides the image table's, or a
    logits GEMM (N = V) of more than 8, would be the GEMM + cell route in caption block 0 or in the 256-row pieces.

    A local build (not kept) whose caption loop read `d_in + off[t]` without `+ j0` PASSED a first version of this test, whose model was
    width_cases.decode_model as it stands: there the fed word moves a score by a hundredth of this bound.  Hence the rescaled model of
    tests/score_blocks_case.py, at which the same misread lies 3.5 bounds away in the median (tests/test_score_blocks_case.py, on the
    CPU) and the same wrong build fails here (pair 12, image 3, caption 179: -36.111 against -32.807, 3.30 > 0.71)."""
    R = ride_along()
    monkeypatch.setenv("LRCN_TRACE_ROUTES", "1")
    capfd.readouterr()
    s = L.score_pairs(R["ctx"], R["param"], L.to_jl(R["feats"]), R["caps"], R["pi"], R["pc"])
    err = capfd.readouterr().err
    monkeypatch.delenv("LRCN_TRACE_ROUTES")
    R["scores"] = s
    assert s.shape == (RA_P,) and np.isfinite(s).all()
    gemms = trace_lines(err)
    gates = sorted(g[0] for g in gemms if g[1] == 4 * R["H"])
    logits = sorted(g[0] for g in gemms if g[1] == R["V"])
    # routed GEMMs of 4 H columns: the token table (V rows), the image table (256 and 4), caption block 1's two recurrent steps (44
    # captions, 36 of them of two words) and the last piece's three (8 pairs of one-word captions: P_0; P_1 and h2).  Nothing of 256 rows
    # besides the image table: caption block 0 and the two 256-row pieces ran the cell epilogue.  Logits: the last piece's two steps.
    assert gates == sorted([R["V"], 256, RA_N - 256, 44, 36, 8, 8, 8]), gates
    assert logits == [8, 8], logits
    pairs = list(zip(R["pi"].tolist(), R["pc"].tolist()))
    ref = oracle_scores(R["m"], R["feats"], R["caps"], pairs, bf16=True)
    gap = 0.0
    for q, (n, c) in enumerate(pairs):
        v = ref[(n, c)]
        gap = max(gap, abs(s[q] - v) / (1 + abs(v)))
    print("bf16, max_B 256: %d pairs, max |gap| / (1 + |s|) = %.3g" % (RA_P, gap))
    for q, (n, c) in enumerate(pairs):
        v = ref[(n, c)]
        assert abs(s[q] - v) <= 5e-2 + 2e-2 * abs(v), (q, n, c, s[q], v)


def test_ride_along_rows_cannot_reach_active_rows_bit_exact():
    """The same call twice on the same context; the second with other (valid) word ids in the 260 short captions, lengths and pairs as they
    were.  A long caption's rows share their launches with the short ones' rows -- active at first, riding along once they have ended -- and
    must not see them: the scores of every pair of a long caption are the same bits.  (The call's GEMMs take their ordered forms.)"""
    R = ride_along()
    fj = L.to_jl(R["feats"])
    a = R.get("scores")
    if a is None:
        a = L.score_pairs(R["ctx"], R["param"], fj, R["caps"], R["pi"], R["pc"])
    rng = np.random.default_rng(44)
    caps2 = [list(c) if len(c) == 6 else [3 + (int(w) - 3 + int(rng.integers(1, R["V"] - 3))) % (R["V"] - 3) for w in c] for c in R["caps"]]
    assert all(len(x) == len(y) and all(3 <= w < R["V"] for w in x) for x, y in zip(caps2, R["caps"]))
    assert all((x == list(y)) == (len(y) == 6) for x, y in zip(caps2, R["caps"]))
    b = L.score_pairs(R["ctx"], R["param"], fj, caps2, R["pi"], R["pc"])
    long_pair = np.array([len(R["caps"][c]) == 6 for c in R["pc"]])
    assert long_pair.sum() >= RA_LONG and (~long_pair).sum() >= RA_SHORT
    assert np.asarray(a, np.float32)[long_pair].tobytes() == np.asarray(b, np.float32)[long_pair].tobytes(), \
        np.abs(np.asarray(a) - np.asarray(b))[long_pair].max()
    assert (np.asarray(a)[~long_pair] != np.asarray(b)[~long_pair]).any()


# ------------------------------------------------------------------------------------------------ 2. bf16, fused route, production width
def test_bf16_production_matches_emulating_oracle():
    P = production()
    caps = P["caps"]
    s = L.score_matrix(P["ctx"], P["param"], L.to_jl(P["feats"]), caps)
    assert s.shape == (NP, MP) and np.isfinite(s).all()
    # captions at every length boundary of the sorted order (first and last of each length), the longest and shortest, and a random few
    order = sorted(range(MP), key=lambda c: -len(caps[c]))
    chosen = {order[0], order[-1]}
    for i in range(1, MP):
        if len(caps[order[i]]) != len(caps[order[i - 1]]):
            chosen |= {order[i], order[i - 1]}
    rng = np.random.default_rng(3)
    chosen |= set(int(c) for c in rng.choice(MP, 8, replace=False))
    pairs = set()
    for c in sorted(chosen):
        pairs |= {(0, c), (NP - 1, c)}
        pairs |= {(int(n), c) for n in rng.choice(NP, 3, replace=False)}
    pairs = sorted(pairs)
    assert len(pairs) >= 200
    ref = oracle_scores(P["m"], P["feats"], caps, pairs, bf16=True)
    gap = 0.0
    for (n, c), v in ref.items():
        gap = max(gap, abs(s[n, c] - v) / (1 + abs(v)))
        assert abs(s[n, c] - v) <= 5e-2 + 2e-2 * abs(v), (n, c, s[n, c], v)
    print("bf16 vs emulating oracle: %d pairs, max |gap| / (1 + |s|) = %.3g" % (len(pairs), gap))


# ------------------------------------------------------------------------------------------------ 3. routes agree
def test_fused_and_unfused_routes_agree(monkeypatch):
    P = production()
    fj = L.to_jl(P["feats"])
    a = L.score_matrix(P["ctx"], P["param"], fj, P["caps"])
    monkeypatch.setenv("LRCN_SCORE_FUSED", "0")
    b = L.score_matrix(P["ctx"], P["param"], fj, P["caps"])
    monkeypatch.delenv("LRCN_SCORE_FUSED")
    steps = step_counts(P["caps"])[None, :]
    gap = np.abs(a - b) / steps
    print("fused vs unfused: max |gap| / (L + 1) = %.3g" % gap.max())
    assert (gap <= 1e-3).all(), gap.max()


# ------------------------------------------------------------------------------------------------ 4. pairs == matrix
def test_pairs_equal_matrix_f32():
    m = small_model(seed=8)
    N, M = 9, 31
    caps = captions_of(M, 203, 9)
    feats = feats_of(N, 4)
    ctx = L.Context(64, 64, 64, 203, max_B=96, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats)
    s = L.score_matrix(ctx, param, fj, caps)
    rng = np.random.default_rng(5)
    pi = rng.integers(0, N, size=250)
    pc = rng.integers(0, M, size=250)
    pi[:3], pc[:3] = [0, N - 1, 4], [M - 1, 0, 4]
    sp = L.score_pairs(ctx, param, fj, caps, pi, pc)
    ctx.close()
    ref = s[pi, pc]
    assert (np.abs(sp - ref) <= 1e-5 * (1 + np.abs(ref))).all(), np.abs(sp - ref).max()


# ------------------------------------------------------------------------------------------------ 5. permutation and repeatability
def _perm_check(ctx, param, feats, caps, seed):
    N, M = feats.shape[0], len(caps)
    s = L.score_matrix(ctx, param, L.to_jl(feats), caps)
    again = L.score_matrix(ctx, param, L.to_jl(feats), caps)
    assert np.array_equal(s, again)
    rng = np.random.default_rng(seed)
    pn, pm = rng.permutation(N), rng.permutation(M)
    sp = L.score_matrix(ctx, param, L.to_jl(np.ascontiguousarray(feats[pn])), [caps[i] for i in pm])
    assert np.array_equal(sp, s[np.ix_(pn, pm)])


def test_permutation_and_repeat_are_bit_identical_f32():
    m = small_model(seed=6)
    ctx = L.Context(64, 64, 64, 203, max_B=50, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    _perm_check(ctx, L.model_from_arrays(m.p), feats_of(8, 2), captions_of(19, 203, 4), 1)
    ctx.close()


def test_permutation_and_repeat_are_bit_identical_bf16_production():
    P = production()
    _perm_check(P["ctx"], P["param"], P["feats"], P["caps"], 2)


# ------------------------------------------------------------------------------------------------ 6. pieces
def test_pieces_of_256_rows_match_one_piece():
    P = production()
    fj = L.to_jl(P["feats"])
    a = L.score_matrix(P["ctx"], P["param"], fj, P["caps"])
    small = L.Context(E, H, H, V, max_B=256, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
    b = L.score_matrix(small, P["param"], fj, P["caps"])
    small.close()
    gap = np.abs(a - b) / step_counts(P["caps"])[None, :]
    print("max_B 256 vs 5120: max |gap| / (L + 1) = %.3g" % gap.max())
    assert (gap <= 1e-3).all(), gap.max()


# ------------------------------------------------------------------------------------------------ 7. against the sampler
def _sampler_check(ctx, param, feats, S, nword, bound_rel, min_ended):
    N = feats.shape[0]
    fj = L.to_jl(feats)
    res = L.sample_batch(ctx, param, fj, S, nword, temperature=1.0, seed=77)
    caps, pi, lps = [], [], []
    for i, draws in enumerate(res):
        for seq, lp in draws:
            if seq[-1] == 0 and len(seq) >= 3:   # [bos, w1 .. wk, eos] with k >= 1
                caps.append([int(t) for t in seq[1:-1]])
                pi.append(i)
                lps.append(lp)
    assert len(caps) >= min_ended, len(caps)
    sc = L.score_pairs(ctx, param, fj, caps, pi, list(range(len(caps))))
    lps = np.array(lps, np.float64)
    gap = np.abs(sc - lps) / (1 + np.abs(lps))
    print("sampler vs scorer: %d draws ended in eos, max |gap| / (1 + |lp|) = %.3g" % (len(caps), gap.max()))
    assert (gap <= bound_rel).all(), gap.max()


def test_scores_reproduce_sampler_loglik_f32():
    m = small_model(seed=12)
    ctx = L.Context(64, 64, 64, 203, max_B=320, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    _sampler_check(ctx, L.model_from_arrays(m.p), feats_of(64, 7), 5, 26, 1e-4, 5)
    ctx.close()


def test_scores_reproduce_sampler_loglik_bf16_production_width():
    # the decisive model never draws eos at temperature 1: an unscaled one at production width with a large eos bias ends most draws early
    m = orc.init_weights(E, H, H, V, seed=14)
    m.p["bout"][0, 0] = 8.0
    ctx = L.Context(E, H, H, V, max_B=NP * 5, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
    _sampler_check(ctx, L.model_from_arrays(m.p), feats_of(NP, 13), 5, 26, 1e-2, 50)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. no side effects on the beam
def test_score_call_leaves_beam_search_unchanged():
    P = production()
    fj = L.to_jl(feats_of(NP, 17))
    before = L.beam_search_batch(P["ctx"], P["param"], fj, 5, 8)
    L.score_matrix(P["ctx"], P["param"], L.to_jl(P["feats"]), P["caps"])
    L.score_pairs(P["ctx"], P["param"], L.to_jl(P["feats"]), P["caps"][:7], [0, 5, 63], [6, 0, 3])
    after = L.beam_search_batch(P["ctx"], P["param"], fj, 5, 8)
    assert before == after


# ------------------------------------------------------------------------------------------------ 8b. scratch reuse
def test_calls_of_other_sizes_on_a_used_context_match_a_fresh_context_bf16():
    """The context's scoring scratch is laid out anew by every call: a small call after a large one (pairs under 256 rows -- GEMM + cell
    kernel route -- a small matrix on the same route, a matrix on the fused route) must give the bits a fresh context gives.  (Bits: the
    calls' GEMMs take their ordered forms, so the under-256-row route repeats exactly too.)"""
    P = production()
    caps, feats = P["caps"], P["feats"]
    rng = np.random.default_rng(31)
    pi, pc = rng.integers(0, NP, size=150), rng.integers(0, 30, size=150)
    calls = [lambda ctx: L.score_pairs(ctx, P["param"], L.to_jl(feats), caps[:30], pi, pc),            # 150 rows
             lambda ctx: L.score_matrix(ctx, P["param"], L.to_jl(feats[:10]), caps[:20]),               # 200 rows
             lambda ctx: L.score_matrix(ctx, P["param"], L.to_jl(feats[:16]), caps[30:60])]             # 480 rows
    L.score_matrix(P["ctx"], P["param"], L.to_jl(feats), caps)   # the large call first
    used = [f(P["ctx"]) for f in calls]
    for f, u in zip(calls, used):
        fresh = L.Context(E, H, H, V, max_B=NP * MP, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        ref = f(fresh)
        fresh.close()
        assert np.isfinite(ref).all()
        assert np.array_equal(u, ref), np.nanmax(np.abs(u - ref))


# ------------------------------------------------------------------------------------------------ 9. argument errors
def test_argument_errors_return_einval():
    m = small_model()
    N, M = 3, 4
    ctx = L.Context(64, 64, 64, 203, max_B=8, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats_of(N, 1))
    lib = _lib.lib()
    Tmax = 5
    out = L.to_jl(np.zeros((N * M, 1), np.float32))

    def arr(a, t=C.c_int32):
        a = np.ascontiguousarray(a, np.int32)
        return a, a.ctypes.data_as(C.POINTER(t))

    good_tok = np.full((Tmax, M), 5, np.int32)
    good_len = np.array([1, 5, 3, 2], np.int32)

    def mat(tok=good_tok, lens=good_len, N_=N, M_=M, T_=Tmax, feats=True, scores=True, h=None):
        t, tp = arr(tok)
        l_, lp_ = arr(lens, C.c_int)
        return lib.lrcn_score_matrix(h or ctx._h, L._p9(param), L._ptr(fj) if feats else None, N_, tp, lp_, M_, T_,
                                     C.c_void_p(out.data_ptr()) if scores else None)

    def pairs(pi, pc, P_=None):
        t, tp = arr(good_tok)
        l_, lp_ = arr(good_len, C.c_int)
        a, ap = arr(pi)
        b, bp = arr(pc)
        return lib.lrcn_score_pairs(ctx._h, L._p9(param), L._ptr(fj), N, tp, lp_, M, Tmax, ap, bp, len(a) if P_ is None else P_,
                                    C.c_void_p(out.data_ptr()))

    assert mat() == 0
    assert pairs([0, 2], [3, 0]) == 0
    bad_tok = good_tok.copy(); bad_tok[4, 1] = 203          # noqa: E702
    neg_tok = good_tok.copy(); neg_tok[0, 0] = -1           # noqa: E702
    ign_tok = good_tok.copy(); ign_tok[4, 0] = 9999         # noqa: E702  (t >= lens[0]: ignored)
    assert mat(tok=ign_tok) == 0
    cases = [dict(N_=0), dict(M_=0), dict(N_=-1), dict(T_=0), dict(feats=False), dict(scores=False),
             dict(tok=bad_tok), dict(tok=neg_tok),
             dict(lens=np.array([0, 5, 3, 2])), dict(lens=np.array([1, 6, 3, 2])), dict(lens=np.array([1, 29, 3, 2]), T_=29)]
    for kw in cases:
        if kw.get("T_") == 29:
            kw["tok"] = np.full((29, M), 5, np.int32)
        assert mat(**kw) == -1, kw
        assert lib.lrcn_last_error(ctx._h)
    assert pairs([0, 3], [0, 0]) == -1       # image out of range
    assert pairs([0, 0], [0, 4]) == -1       # caption out of range
    assert pairs([0, -1], [0, 0]) == -1
    assert pairs([0], [0], P_=0) == -1
    t, tp = arr(good_tok)
    l_, lp_ = arr(good_len, C.c_int)
    assert lib.lrcn_score_pairs(ctx._h, L._p9(param), L._ptr(fj), N, tp, lp_, M, Tmax, None, None, 1, C.c_void_p(out.data_ptr())) == -1
    assert lib.lrcn_score_matrix(None, L._p9(param), L._ptr(fj), N, tp, lp_, M, Tmax, C.c_void_p(out.data_ptr())) == -1
    ctx.close()
    one = L.Context(64, 64, 64, 203, max_B=8, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=1)
    m1 = small_model(n_layers=1)
    p1 = L.model_from_arrays(m1.p)
    assert lib.lrcn_score_matrix(one._h, L._p9(p1), L._ptr(fj), N, tp, lp_, M, Tmax, C.c_void_p(out.data_ptr())) == -1
    one.close()
