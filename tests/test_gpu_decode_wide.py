"""GPU: the decode routes that hang on the beam width, the vocabulary size and the float32 range -- each a few lines away from a route the
other decode tests pin, each checked against the CPU oracle (oracle/oracle.py, tests/nbest_ref.py, tests/philox_ref.py):

1. the reference beam at K = 6..32 (softmax_topk_rows_kernel + beam_update_kernel's K*K ranking instead of the fused K <= 5 epilogue), f32,
   exact tokens, on two-layer and LRCN-1f models, at every softmax_topk_rows_kernel<Q> boundary of V;
2. the same widths at the production shape in bf16 (cell epilogue and input-projection tables on), across LRCN_DECODE_EPI / _TABLES;
3. the underflow regime of the reference beam (lrcn.jl:658 multiplies float32 probabilities): products that go subnormal and then 0, where
   every candidate ties and the stable order alone picks the caption -- p compared bit for bit;
4. vocabularies past softmax_topk_rows_kernel's limit (16384), sample_rows_kernel's LDS staging (15360) and the records merges' 256 records
   (V = 32768): every call returns and agrees with the oracle and with the other route;
5. a tie group (distinct logits, one float probability) larger than the 64 entries softmax_topk_rows_kernel's rounds visit."""
import os
import sys

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import lrcn as L
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nbest_ref as nb  # noqa: E402
import philox_ref as ph  # noqa: E402

pytestmark = pytest.mark.gpu

EOS, BOS = lrcn_amd.EOS, lrcn_amd.BOS
FLT_MIN = float(np.finfo(np.float32).tiny)


def feats_of(N, seed):
    return (np.random.default_rng(seed).standard_normal((N, 4096)) * 0.05).astype(np.float32)


def peaked_model(E, V, seed, n_layers=2, spread=16.0, eos_rel=None):
    """As test_gpu_decode_epilogue.py's decisive model at small widths: scaled weights and a random bout make the word distributions peaky,
    so no near-tie separates the GPU's and the oracle's sums.  eos_rel: eos's bias relative to the largest other bias."""
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, E, E, V, seed=seed, n_layers=n_layers)
    for n in ("W1", "W2"):
        m.p[n] *= 2.0
    m.p["Wout"][:] *= spread
    m.p["bout"][:] = (rng.standard_normal((1, V)) * 2.0).astype(np.float32)
    if eos_rel is not None:
        m.p["bout"][0, EOS] = m.p["bout"][0, 1:].max() + eos_rel
    return m


def oracle_beam(m, feat, K, nword, bf16=False):
    if bf16:
        with orc.emulate_bf16():
            t, p = orc.beam_search(m, feat, K, nword)
    else:
        t, p = orc.beam_search(m, feat, K, nword)
    return list(t), p


def same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. wide reference beam, f32, against the oracle
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("K", [6, 8, 10, 16, 32])
def test_wide_beam_f32_equals_oracle(K, n_layers):
    """Both entry points against orc.beam_search at K >= SMAX_KC, on an eos-bias sweep: captions that stop at once, at mixed lengths and only
    at the nword limit, so frozen and live images share the batched decode."""
    E, V, nword, N = 48, 157, 10, 6
    feats = feats_of(N, 100 + K)
    ctx = L.Context(E, E, E, V, max_B=N * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)
    lens, mixed = set(), 0
    for eos_bias in (3.0, 0.0, -0.3, -3.0):
        m = peaked_model(E, V, seed=10 + K, n_layers=n_layers, eos_rel=eos_bias)
        param = L.model_from_arrays(m.p)
        batch = L.beam_search_batch(ctx, param, L.to_jl(feats), K, nword)
        for i in range(N):
            rt, rp = oracle_beam(m, feats[i], K, nword)
            one = L.beam_search(ctx, param, L.to_jl(feats[i:i + 1]), K, nword)
            for label, (t, p) in (("per image", one), ("batched", batch[i])):
                assert t == rt, (label, eos_bias, i, t, rt)
                assert abs(p - rp) <= 1e-4 * abs(rp), (label, eos_bias, i, p, rp)
            lens.add(len(rt))
        mixed += len(set(len(t) for t, _ in batch)) > 1
    ctx.close()
    assert min(lens) == 2 and max(lens) == nword + 2 and mixed, (lens, mixed)


@pytest.mark.parametrize("V", [4096, 4097, 8192, 8193, 12288, 12289, 16384])
def test_k32_beam_at_the_rows_kernel_instantiation_boundaries(V):
    """softmax_topk_rows_kernel<Q> holds 4 Q columns per thread: Q = 4, 8, 12, 16 up to V = 4096, 8192, 12288, 16384.  K = 32 on each side."""
    E, K, nword, N = 32, 32, 6, 2
    m = peaked_model(E, V, seed=V, eos_rel=-3.0)
    feats = feats_of(N, V)
    ctx = L.Context(E, E, E, V, max_B=N * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    batch = L.beam_search_batch(ctx, param, L.to_jl(feats), K, nword)
    for i in range(N):
        rt, rp = oracle_beam(m, feats[i], K, nword)
        one = L.beam_search(ctx, param, L.to_jl(feats[i:i + 1]), K, nword)
        for label, (t, p) in (("per image", one), ("batched", batch[i])):
            assert t == rt, (label, i, t, rt)
            assert abs(p - rp) <= 1e-4 * abs(rp), (label, i, p, rp)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. wide beam at the production shape, bf16
EP, VP, NWP = 1000, 10640, 8
_production = {}


def production():
    """As tests/test_gpu_decode_epilogue.py's decisive model: peaky distributions at E = H = 1000, V = 10640; one context of 5120 rows."""
    if not _production:
        rng = np.random.default_rng(4)
        m = orc.init_weights(EP, EP, EP, VP, seed=4)
        for n in ("W1", "W2", "Wout"):
            m.p[n] *= 2.0
        m.p["Wout"][:] *= 8.0
        m.p["bout"][:] = (rng.standard_normal((1, VP)) * 2.0).astype(np.float32)
        m.p["b1"][:] += (rng.standard_normal(m.p["b1"].shape) * 0.5).astype(np.float32)
        ctx = L.Context(EP, EP, EP, VP, max_B=5120, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
        _production.update(m=m, ctx=ctx, param=L.model_from_arrays(m.p))
    return _production


def teardown_module(module):
    if _production:
        _production["ctx"].close()
        _production.clear()


def compare_routes(a, b, N):
    """As test_gpu_decode_epilogue.py: >= 98 % identical captions (a near-tie may fall the other way under another summation order)."""
    same = sum(x[0] == y[0] for x, y in zip(a, b))
    assert same >= N - N // 50, (same, N)
    for (ta, pa), (tb, pb) in zip(a, b):
        if ta == tb:
            assert abs(pa - pb) <= 2e-2 * abs(pb) + 1e-30, (pa, pb)
        else:
            assert abs(np.log(pa + 1e-300) - np.log(pb + 1e-300)) < 0.3, (pa, pb)


@pytest.mark.parametrize("K,N", [(10, 512), (32, 160)])
def test_wide_beam_production_bf16(K, N, monkeypatch):
    P = production()
    feats = feats_of(N, 200 + K)
    fj = L.to_jl(feats)
    out = {}
    for epi, tables in (("1", "1"), ("1", "0"), ("0", "1")):   # tables need the cell epilogue: EPI=0 is the plain [x | h] route
        monkeypatch.setenv("LRCN_DECODE_EPI", epi)
        monkeypatch.setenv("LRCN_DECODE_TABLES", tables)
        out[epi + tables] = L.beam_search_batch(P["ctx"], P["param"], fj, K, NWP)
    monkeypatch.delenv("LRCN_DECODE_EPI")
    monkeypatch.delenv("LRCN_DECODE_TABLES")
    base = out["11"]
    assert L.beam_search_batch(P["ctx"], P["param"], fj, K, NWP) == base   # repeats itself
    compare_routes(out["10"], base, N)
    compare_routes(out["01"], base, N)
    picks = [0, 1, N // 2, N - 1]
    agree = 0
    for i in picks:   # the per-image decode (K rows, no epilogue): its own GEMM shapes
        t, p = L.beam_search(P["ctx"], P["param"], L.to_jl(feats[i:i + 1]), K, NWP)
        if t == base[i][0]:
            agree += 1
            assert abs(p - base[i][1]) <= 2e-2 * abs(p) + 1e-30, (i, p, base[i][1])
    assert agree >= len(picks) - 1, agree
    for i in ([0, N - 1] if K == 10 else [N // 2]):   # the emulating oracle: few calls, they are the cost
        rt, rp = oracle_beam(P["m"], feats[i], K, NWP, bf16=True)
        assert base[i][0] == rt, (i, base[i][0], rt)
        assert abs(base[i][1] - rp) <= 5e-2 * abs(rp) + 1e-30, (i, base[i][1], rp)


# ------------------------------------------------------------------------------------------------ 3. the underflow regime
EU, VU = 64, 997


def flat_tied_model(seed=31, group=40, V=VU, E=EU):
    """Wout = 0: the logits are bout exactly, the same for every hypothesis.  `group` words share the largest logit exactly, so every one of
    the K*K candidates of a step has the same probability product -- first a normal number, then subnormal, then 0 -- and the stable
    order alone (ties: lower candidate index, lower column) picks the caption.  eos is suppressed: the decodes run to nword."""
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, E, E, V, seed=seed)
    m.p["Wout"][:] = 0.0
    bout = np.clip(rng.standard_normal(V) * 0.3, -1.2, 1.2).astype(np.float32)   # all below the group's 1.5
    top = rng.choice(np.arange(3, V), size=group, replace=False)
    bout[top] = np.float32(1.5)
    bout[EOS] = -30.0
    m.p["bout"][:] = bout[None, :]
    return m


def flat_random_model(seed=32):
    """Small random Wout: nearly flat distributions that differ between hypotheses, so the states -- and which parent a hypothesis
    continues -- still decide the ranking; the products underflow just the same.  eos is suppressed."""
    rng = np.random.default_rng(seed)
    m = orc.init_weights(EU, EU, EU, VU, seed=seed)
    m.p["Wout"][:] *= 1.5
    m.p["bout"][:] = (rng.standard_normal((1, VU)) * 0.3).astype(np.float32)
    m.p["bout"][0, EOS] = -30.0
    return m


# (model, nword that ends subnormal, nword that ends at 0 after >= 3 steps at 0).  The oracle's numbers confirm each regime in the test.
VW = 16392   # past softmax_topk_rows_kernel's V limit: softmax_rows_kernel + topk_rows_kernel, whose tie rule then picks every word
UNDERFLOW = {"tied": (flat_tied_model, 17, 22), "random": (flat_random_model, 16, 21), "tied-wide": (lambda: flat_tied_model(V=VW), 11, 15)}


def underflow_refs(m, feats, K, sub_n, zero_n, bf16=False):
    """Oracle decodes at the two nwords (and at zero_n - 3, to show that the zeros held for several steps); asserts both regimes."""
    refs = {}
    for i, f in enumerate(feats):
        a = oracle_beam(m, f, K, sub_n, bf16)
        b = oracle_beam(m, f, K, zero_n, bf16)
        c = oracle_beam(m, f, K, zero_n - 3, bf16)
        assert 0.0 < a[1] < FLT_MIN, ("not subnormal", K, i, a[1])
        assert b[1] == 0.0 and c[1] == 0.0, ("did not reach 0 early", K, i, b[1], c[1])   # best = 0: all K*K candidates tie at 0
        refs[(i, sub_n)], refs[(i, zero_n)] = a, b
    return refs


def check_underflow(got, ref, label):
    t, p = got
    rt, rp = ref
    assert t == rt, (label, t, rt)
    if rp == 0.0 or rp < FLT_MIN:
        assert same_bits(p, rp), (label, p, rp)
    else:
        assert abs(p - rp) <= 1e-4 * rp, (label, p, rp)


@pytest.mark.parametrize("kind", ["tied", "random", "tied-wide"])
@pytest.mark.parametrize("K", [1, 3, 5, 6, 10, 32])
def test_underflow_f32_equals_oracle(kind, K):
    make, sub_n, zero_n = UNDERFLOW[kind]
    m = make()
    feats = feats_of(3, 300 + K)
    refs = underflow_refs(m, feats, K, sub_n, zero_n)
    ctx = L.Context(EU, EU, EU, m.V, max_B=3 * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    for nword in (sub_n, zero_n):
        batch = L.beam_search_batch(ctx, param, L.to_jl(feats), K, nword)
        for i in range(len(feats)):
            check_underflow(L.beam_search(ctx, param, L.to_jl(feats[i:i + 1]), K, nword), refs[(i, nword)], (kind, K, nword, i, "per image"))
            check_underflow(batch[i], refs[(i, nword)], (kind, K, nword, i, "batched"))
    ctx.close()


EB, VB = 128, 1000   # bf16: H2 > 64 and V % 4 == 0, so that from 256 rows the logits GEMM may reduce to records (smax_records_on)


@pytest.mark.parametrize("K,smax", [(1, "1"), (3, "1"), (5, "1"), (5, "0"), (6, "1"), (10, "1"), (32, "1")])
def test_underflow_bf16_equals_emulating_oracle(K, smax, monkeypatch):
    """bf16 on the tied model (logits = bout whatever the state: the bf16 routes' rounding cannot move a tie) at E = H = 128, V = 1000, from
    256 rows: at K <= 5 the logits GEMM's softmax / top-K records and their merge (GEMM_OUT_SMAX_TOPK, softmax_topk_merge_kernel), whose
    records keep SMAX_KC = 6 candidates of 128 columns each while the 40-word tie group puts up to 9 words into one record; at K >= 6 and
    with LRCN_DECODE_SMAX=0 the f32 logits and softmax_topk_rows_kernel.  Every image decodes the same caption."""
    make, sub_n, zero_n = UNDERFLOW["tied"]
    m = flat_tied_model(V=VB, E=EB)
    g = np.flatnonzero(m.p["bout"][0] == m.p["bout"][0].max())
    assert np.bincount(2 * (g // 256) + (g % 64 >= 32)).max() > 6   # records of 128 columns (alternating runs of 32 of a 256-column tile)
    f1 = feats_of(1, 400 + K)
    refs = underflow_refs(m, f1, K, sub_n, zero_n, bf16=True)
    N = max(2, -(-256 // K))
    assert N * K >= 256 and EB > 64 and VB % 4 == 0 and 2 * -(-VB // 256) <= 256   # the records route is eligible; smax picks it or not
    feats = feats_of(N, 401 + K)
    ctx = L.Context(EB, EB, EB, VB, max_B=N * K, max_T=2, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.model_from_arrays(m.p)
    monkeypatch.setenv("LRCN_DECODE_SMAX", smax)
    for nword in (sub_n, zero_n):
        ref = refs[(0, nword)]
        batch = L.beam_search_batch(ctx, param, L.to_jl(feats), K, nword)
        for i in range(N):
            check_underflow(batch[i], ref, (K, smax, nword, i, "batched"))
        check_underflow(L.beam_search(ctx, param, L.to_jl(feats[:1]), K, nword), ref, (K, nword, "per image"))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. vocabularies past every limit
E4 = 128   # H2 > 64: the record epilogues are eligible where V allows


@pytest.mark.parametrize("V", [15361, 16385, 32768, 33024])
def test_large_vocabulary_f32_beam_and_nbest_equal_oracle(V):
    """f32: the beam at K = 5 and 10 (above 16384 softmax_rows_kernel + topk_rows_kernel) and n-best against nbest_ref
    (log_softmax_rows_kernel + topk_rows_kernel above 16384)."""
    nword, N = 6, 2
    m = peaked_model(E4, V, seed=V + 1, eos_rel=-0.3)
    feats = feats_of(N, V + 2)
    ctx = L.Context(E4, E4, E4, V, max_B=N * 10, max_T=2, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    fj = L.to_jl(feats)
    for K in (5, 10):
        batch = L.beam_search_batch(ctx, param, fj, K, nword)
        for i in range(N):
            rt, rp = oracle_beam(m, feats[i], K, nword)
            one = L.beam_search(ctx, param, L.to_jl(feats[i:i + 1]), K, nword)
            for label, (t, p) in (("per image", one), ("batched", batch[i])):
                assert t == rt, (V, K, label, i, t, rt)
                assert abs(p - rp) <= 1e-4 * abs(rp), (V, K, label, i, p, rp)
    K = 5
    gpu = L.beam_nbest_batch(ctx, param, fj, K, nword, 1.0)
    ref = nb.search(nb.OracleStep(orc, m, feats), N, K, nword, 1.0)
    ctx.close()
    for i, (g, r) in enumerate(zip(gpu, ref)):
        assert [e[0] for e in g] == [list(e[0]) for e in r], (V, i)
        for (_, glp, gsc), (_, rlp, rsc) in zip(g, r):
            assert abs(glp - float(rlp)) <= 1e-4 * (1 + abs(float(rlp))), (V, i, glp, rlp)
            assert abs(gsc - float(rsc)) <= 1e-4 * (1 + abs(float(rsc))), (V, i, gsc, rsc)


def sample_replay(m, feats, res, S, T, top_k, seed, rows):
    """As tests/test_gpu_sample.py: teacher-forced through the emulating oracle, every GPU token is an admitted column whose z / T + g is
    within delta of the host maximum, and the log-likelihood is the host sum of log softmax(z)[token].  Returns (exact steps, steps)."""
    fl = [row for img in res for row in img]
    Tn = max(max(len(fl[r][0]) for r in rows) - 2, 1)
    toks = np.zeros((Tn, len(rows)), np.int32)
    for b, r in enumerate(rows):
        seq = fl[r][0]
        for t in range(len(seq) - 2):
            toks[t, b] = seq[t + 1]
    with orc.emulate_bf16():
        z_all = orc.forward_logits(m, np.stack([feats[r // S] for r in rows]), toks)
    exact = steps = 0
    for b, r in enumerate(rows):
        seq, lp = fl[r]
        host_lp = 0.0
        for t in range(len(seq) - 1):
            z, tok = z_all[t, b], seq[t + 1]
            cols, sc = ph.scores(z, T, top_k, seed, r // S, r % S, t + 1)
            best = float(sc.max())
            assert tok in cols, (r, t, tok)
            assert float(sc[list(cols).index(tok)]) >= best - 2e-2 * (1.0 + abs(best)), (r, t, tok)
            exact += int(cols[int(np.argmax(sc))] == tok)
            steps += 1
            host_lp += ph.log_softmax(z)[tok]
        assert abs(lp - host_lp) <= 5e-2 + 2e-2 * abs(host_lp), (r, lp, host_lp)
    return exact, steps


def score_oracle(m, feats, caps, pairs):
    """s(n, c) = sum of log softmax(z)[word] over the words and eos, z from the emulating oracle (tests/test_gpu_score.py)."""
    out = {}
    by_len = {}
    for n, c in pairs:
        by_len.setdefault(len(caps[c]), []).append((n, c))
    for Lc, group in by_len.items():
        toks = np.array([caps[c] for _, c in group], np.int32).T.reshape(Lc, len(group))
        with orc.emulate_bf16():
            z = orc.forward_logits(m, np.stack([feats[n] for n, _ in group]), toks).astype(np.float64)
        lp = z - (z.max(axis=2, keepdims=True) + np.log(np.exp(z - z.max(axis=2, keepdims=True)).sum(axis=2, keepdims=True)))
        for b, (n, c) in enumerate(group):
            y = list(caps[c]) + [EOS]
            out[(n, c)] = float(sum(lp[t, b, y[t]] for t in range(Lc + 1)))
    return out


@pytest.mark.parametrize("V", [8192, 8196, 15361, 16384, 16385, 16388, 32768, 33024])
def test_large_vocabulary_bf16_record_routes_against_row_routes_and_oracle(V, monkeypatch):
    """bf16 from 256 rows, where the logits GEMM reduces to records when V % 4 == 0 and no more than 256 records make a row (V <= 32768):
    beam, n-best, sampling (top_k 0 and 3) and scoring on the default route against LRCN_DECODE_SMAX=0 / LRCN_SCORE_FUSED=0 and the
    emulating oracle.  At V = 33024 (258 records) every call must still return: the default route is then the f32-logits one.
    V = 8192 | 8196 and 16384 | 16388: 64 | 66 and 128 | 130 records per row, both sides of the <1> | <2> | <4> instantiations of
    softmax_topk_merge_kernel, sample_gumbel_merge_kernel, sample_topk_merge_kernel and score_pick_merge_kernel (tests/INSTANTIATIONS.md)."""
    K, nword = 5, 5
    N = 52   # 260 rows: beam, n-best and K = 5 samples per image
    m = peaked_model(E4, V, seed=V + 3, eos_rel=-0.3)
    feats = feats_of(N, V + 4)
    fj = L.to_jl(feats)
    ctx = L.Context(E4, E4, E4, V, max_B=N * K, max_T=8, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.model_from_arrays(m.p)
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("LRCN_DECODE_SMAX", knob)
        out[knob] = dict(beam=L.beam_search_batch(ctx, param, fj, K, nword),
                         nbest=L.beam_nbest_batch(ctx, param, fj, K, nword, 0.0),
                         s0=L.sample_batch(ctx, param, fj, K, nword, temperature=1.0, top_k=0, seed=V),
                         s3=L.sample_batch(ctx, param, fj, K, nword, temperature=1.0, top_k=3, seed=V + 1))
    monkeypatch.delenv("LRCN_DECODE_SMAX")
    a, b = out["1"], out["0"]
    compare_routes(a["beam"], b["beam"], N)
    same = sum([e[0] for e in x] == [e[0] for e in y] for x, y in zip(a["nbest"], b["nbest"]))
    assert same >= N - N // 50, (same, N)
    for x, y in zip(a["nbest"], b["nbest"]):
        if [e[0] for e in x] == [e[0] for e in y]:
            for (_, la, _), (_, lb, _) in zip(x, y):
                assert abs(la - lb) <= 1e-3 * (1 + abs(lb)), (la, lb)
    R = N * K
    for key in ("s0", "s3"):
        fa = [r for img in a[key] for r in img]
        fb = [r for img in b[key] for r in img]
        same = sum(x[0] == y[0] for x, y in zip(fa, fb))
        assert same >= R - R // 50, (key, same, R)
    for i in (0, N - 1):   # the emulating oracle's per-image beam
        rt, rp = oracle_beam(m, feats[i], K, nword, bf16=True)
        assert a["beam"][i][0] == rt, (V, i, a["beam"][i][0], rt)
        assert abs(a["beam"][i][1] - rp) <= 5e-2 * abs(rp) + 1e-30
    rows = [0, 1, K + 2, R // 2, R - 1]
    for key, top_k, seed in (("s0", 0, V), ("s3", 3, V + 1)):
        for route in ("1", "0"):
            exact, steps = sample_replay(m, feats, out[route][key], K, 1.0, top_k, seed, rows)
            assert exact >= steps - 1, (V, key, route, exact, steps)
    # scoring: 26 images x 12 captions = 312 rows per step
    rng = np.random.default_rng(V)
    caps = [list(rng.integers(3, V, size=int(n))) for n in rng.integers(1, 7, size=12)]
    sf = feats[:26]
    fused = L.score_matrix(ctx, param, L.to_jl(sf), caps)
    monkeypatch.setenv("LRCN_SCORE_FUSED", "0")
    plain = L.score_matrix(ctx, param, L.to_jl(sf), caps)
    monkeypatch.delenv("LRCN_SCORE_FUSED")
    ctx.close()
    steps = np.array([len(c) + 1 for c in caps], np.float64)[None, :]
    assert (np.abs(fused - plain) / steps <= 1e-3).all(), np.abs(fused - plain).max()
    pairs = [(n, c) for n in (0, 7, 25) for c in range(len(caps))]
    ref = score_oracle(m, sf, caps, pairs)
    for (n, c), v in ref.items():
        assert abs(fused[n, c] - v) <= 5e-2 + 2e-2 * abs(v), (V, n, c, fused[n, c], v)


# ------------------------------------------------------------------------------------------------ 5. a tie group wider than 64 entries
@pytest.mark.parametrize("K", [1, 6, 32])
def test_tie_group_wider_than_the_rows_kernel_rounds(K, monkeypatch):
    """Wout = 0, so the logits are bout exactly.  80 words 100..179 get logits x, x + 1 ulp, ..., x + 79 ulps -- increasing with the index,
    one float32 probability.  The reference keeps the LOWEST indices of that tie group (a stable sort of the probabilities), 100 .. 100+K-1;
    softmax_topk_rows_kernel's rounds visit candidates by descending logit and stop after 64 entries, which hold only 116 .. 179."""
    E, V, nword = 32, 600, 3
    m = orc.init_weights(E, E, E, V, seed=2)
    m.p["Wout"][:] = 0.0
    bout = np.full(V, -4.0, np.float32)
    bout[EOS] = -9.0
    x = np.float32(1e-3)
    for j in range(100, 180):
        bout[j] = x
        x = np.nextafter(x, np.float32(1.0))
    m.p["bout"][:] = bout[None, :]
    lse = np.log(np.exp(bout.astype(np.float64)).sum())
    pf = np.exp(bout.astype(np.float64) - lse).astype(np.float32)
    assert len(set(bout[100:180].tolist())) == 80 and len(set(pf[100:180].tolist())) == 1, "the engineered logits no longer tie in float32"
    feat = feats_of(1, 5)
    rt, rp = oracle_beam(m, feat[0], K, nword)
    assert rt == [BOS] + [100] * (nword + 1), rt
    ctx = L.Context(E, E, E, V, max_B=4 * K, max_T=1, lstm_dtype=lrcn_amd.LRCN_F32)
    param = L.model_from_arrays(m.p)
    t, p = L.beam_search(ctx, param, L.to_jl(feat), K, nword)
    assert t == rt and abs(p - rp) <= 1e-5 * rp, (t, p, rt, rp)
    for i, (t, p) in enumerate(L.beam_search_batch(ctx, param, L.to_jl(np.repeat(feat, 4, axis=0)), K, nword)):
        assert t == rt and abs(p - rp) <= 1e-5 * rp, (i, t, p, rt, rp)
    ctx.close()
