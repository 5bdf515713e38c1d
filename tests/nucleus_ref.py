"""Host restatement of the nucleus (top-p) / any-top_k selection of include/lrcn_nucleus.h, in float64, on top of the noise of
tests/philox_ref.py -- and the fixtures that the CPU and GPU tests of the selection share (rows built BY CONSTRUCTION from chosen shares, so
that the intended nucleus size is decisive: every prefix share is far from top_p)."""
import numpy as np

import philox_ref as ph


def rank_order(z):
    """Columns of a row in rank order: larger z first, lower column first among equal z."""
    z = np.asarray(z)
    return np.lexsort((np.arange(z.shape[0]), -z))


def nucleus_size(z, T, top_k, top_p):
    """(n, G): the admitted set's size and the float64 cumulative share in rank order of the top_k-renormalised distribution, G[m] = share of
    the first m columns of A_k (G[0] = 0, G[|A_k|] = 1).  top_p = 1: n = |A_k| (no mass is looked at)."""
    z = np.asarray(z, dtype=np.float32)
    V = z.shape[0]
    k = V if top_k == 0 else top_k
    ak = rank_order(z)[:k]
    z64 = z.astype(np.float64)
    w = np.exp((z64[ak] - z64.max()) / float(T))
    G = np.concatenate(([0.0], np.cumsum(w) / w.sum()))
    if top_p >= 1.0:
        return k, G
    n = int(np.argmax(G[1:] >= top_p)) + 1 if (G[1:] >= top_p).any() else k
    return n, G


def admitted(z, T, top_k, top_p, n=None):
    """The admitted columns (ascending): the first n of the rank order (n from nucleus_size unless given, e.g. the device's own count)."""
    z = np.asarray(z, dtype=np.float32)
    if n is None:
        n = nucleus_size(z, T, top_k, top_p)[0]
    return np.sort(rank_order(z)[:n])


def scores(z, T, top_k, top_p, seed, i, s, current, n=None):
    """(columns, z / T + g) over the admitted columns, float32 as philox_ref.scores."""
    z = np.asarray(z, dtype=np.float32)
    cols = admitted(z, T, top_k, top_p, n)
    return cols, z[cols] / np.float32(T) + ph.noise(seed, i, s, current, cols)


def draw(z, T, top_k, top_p, seed, i, s, current, n=None):
    cols, sc = scores(z, T, top_k, top_p, seed, i, s, current, n)
    return int(cols[np.argmax(sc)])


def excused(sc):
    """A draw the f32 device may decide the other way: the host's best and second-best scores lie within 1e-4 * (1 + |best|) (the f32 figure
    of tests/test_gpu_sample.py: the device's logf differs from numpy's in the last bits)."""
    if sc.shape[0] < 2:
        return False
    top2 = np.partition(sc.astype(np.float64), -2)[-2:]
    return bool(top2[1] - top2[0] <= 1e-4 * (1.0 + abs(top2[1])))


# ------------------------------------------------------------------------------------------------ fixtures by construction
STAGE_BOUNDARY_V = (15360, 15361)   # at these widths every decisive row's largest share sits in the LAST column: a staged copy of the row that
#                                     drops its last element loses the row maximum (the n* = 1 rows then draw nothing else)
GAP = 6e-3           # every prefix share of a decisive row is at least this far from its top_p
HEAD = 60            # distinct, decreasing head shares, each >= MIN_SHARE; the rest of the mass is spread over the tail
MIN_SHARE = 0.012


def _row_from_shares(shares, T, rng, top_at=None):
    """z = T log(share) scattered over the columns by a seeded permutation; returns (z f32, perm) with column perm[m] holding rank m.
    top_at: the column that holds rank 0 (the permutation's own holder of rank 0 takes that column's rank)."""
    V = shares.shape[0]
    perm = rng.permutation(V)
    if top_at is not None:
        j = int(np.nonzero(perm == top_at)[0][0])
        perm[0], perm[j] = perm[j], perm[0]
    z = np.empty(V, np.float32)
    z[perm] = (float(T) * np.log(shares)).astype(np.float32)
    return z, perm


def head_shares(V, rng, head=HEAD):
    """Shares of one row, in rank order: `head` distinct decreasing shares >= MIN_SHARE, then a tail of smaller ones.  head = V: no tail, the
    mass left over is spread over the head (V = 37: every share >= MIN_SHARE)."""
    h = MIN_SHARE + np.sort(rng.uniform(0.0005, 0.004, head))[::-1]
    if head == V:
        extra = np.sort(rng.uniform(0.5, 1.5, V))[::-1]
        return h + extra / extra.sum() * (1.0 - h.sum())
    t = rng.uniform(0.5, 1.5, V - head)
    t *= (1.0 - h.sum()) / t.sum()
    assert t.max() < 0.8 * MIN_SHARE, t.max()
    return np.concatenate((h, t))


def decisive_row(V, T, n_star, rng):
    """(z, top_p, n_star): top_p in the middle of the gap below the intended boundary -- between the shares of the first n_star - 1 and of the
    first n_star columns -- and the gap asserted in float64 on the f32 logits the device will read."""
    sh = head_shares(V, rng, head=min(HEAD, V))
    z, _ = _row_from_shares(sh, T, rng, top_at=V - 1 if V in STAGE_BOUNDARY_V else None)
    G = nucleus_size(z, T, 0, 1.0)[1]
    top_p = float(np.float32(0.5 * (G[n_star - 1] + G[n_star])))
    assert top_p < 1.0
    n, G = nucleus_size(z, T, 0, top_p)
    assert n == n_star, (n, n_star)
    assert np.abs(G - top_p).min() >= GAP, (V, T, n_star, np.abs(G - top_p).min())
    return z, top_p, n_star


def n_stars(V):
    return [1, 2, 10, 17, 23, 31, 37] if V == 37 else [1, 2, 10, 17, 23, 31, 42, 55, 60]


def tie_row_top_p(V, T, rng, lead=5, tied=8, need=3):
    """A row whose nucleus needs `need` of `tied` columns that share one logit: `lead` distinct shares above them, the tail below.  Returns
    (z, top_p, n_star = lead + need, tied columns ascending)."""
    h = np.array([0.2, 0.15, 0.1, 0.07, 0.05][:lead])
    sh = np.concatenate((h, np.full(tied, 0.04)))
    t = rng.uniform(0.5, 1.5, V - lead - tied)
    t *= (1.0 - sh.sum()) / t.sum()
    assert t.max() < 0.03
    z, perm = _row_from_shares(np.concatenate((sh, t)), T, rng)
    tcols = np.sort(perm[lead:lead + tied])
    assert len(set(z[tcols].tolist())) == 1
    G = nucleus_size(z, T, 0, 1.0)[1]
    top_p = float(np.float32(0.5 * (G[lead + need - 1] + G[lead + need])))
    n, G = nucleus_size(z, T, 0, top_p)
    assert n == lead + need and np.abs(G - top_p).min() >= GAP
    return z, top_p, n, tcols


def tie_row_top_k(V, T, rng, top_k=40, lead=35, tied=8):
    """A row whose top_k boundary falls inside `tied` columns of one logit value (top_k - lead of them are admitted)."""
    h = MIN_SHARE + 0.004 + np.sort(rng.uniform(0.0005, 0.004, lead))[::-1]
    sh = np.concatenate((h, np.full(tied, MIN_SHARE)))
    t = rng.uniform(0.5, 1.5, V - lead - tied)
    t *= (1.0 - sh.sum()) / t.sum()
    assert t.max() < 0.8 * MIN_SHARE
    z, perm = _row_from_shares(np.concatenate((sh, t)), T, rng)
    tcols = np.sort(perm[lead:lead + tied])
    assert len(set(z[tcols].tolist())) == 1 and lead < top_k < lead + tied
    return z, top_k, tcols


COMBO_N = (36, 40, 44)   # intended renormalised sizes of combo_row (where the scale of the later shares stays in (0.2, 1])


def combo_row(V, T, n_star, rng, top_k=50, top_p=0.9):
    """A decisive row for top_k = 50 with top_p = 0.9: 50 head shares, those after rank n_star scaled so that 0.9 of the top-50 mass falls in
    the middle of the share of rank n_star.  Returns (z, n_star)."""
    h = MIN_SHARE + np.sort(rng.uniform(0.0005, 0.004, top_k))[::-1]
    A, s, B = h[:n_star - 1].sum(), h[n_star - 1], h[n_star:].sum()
    f = ((A + 0.5 * s) / top_p - A - s) / B
    assert 0.2 < f <= 1.0, (n_star, f)
    h[n_star:] *= f
    t = rng.uniform(0.2, 0.6, V - top_k) * h.min()   # (unnormalised shares: the tail only has to rank below the 50)
    z, _ = _row_from_shares(np.concatenate((h, t)), T, rng)
    n, G = nucleus_size(z, T, top_k, top_p)
    assert n == n_star and np.abs(G - top_p).min() >= GAP, (n, n_star, np.abs(G - top_p).min())
    return z, n_star


def natural_rows(V, seed, per_std=3):
    """z = std * N(0, 1), std in {1, 3}: nuclei from a few columns to over a thousand."""
    rng = np.random.default_rng(seed)
    return np.stack([(std * rng.standard_normal(V)).astype(np.float32) for std in (1.0, 3.0) for _ in range(per_std)])


def check_draws(z_rows, S, T, top_k, top_p, seed, current, counts=None):
    """Host draws of rows r (image r // S, sample r % S): (tokens, excused flags).  counts: take the admitted set from these sizes."""
    toks, exc = [], []
    for r, z in enumerate(z_rows):
        cols, sc = scores(z, T, top_k, top_p, seed, r // S, r % S, current, None if counts is None else int(counts[r]))
        toks.append(int(cols[np.argmax(sc)]))
        exc.append(excused(sc))
    return np.array(toks), np.array(exc)


# ------------------------------------------------------------------------------------------------ the decisive set of the exact-size test
# below the thread count and odd; several columns per thread; the production width; the last staged and the first unstaged width (k_sample_nucleus
# keeps a row of up to 15360 logits in LDS); unstaged
DECISIVE_V = (37, 203, 10640, 15360, 15361, 16411)
DECISIVE_T = (1.0, 0.7)
DECISIVE_S = 4                         # samples per row: every case is one call of S rows of the same logits
DECISIVE_SEED = 0x5EED0123456789AB
_decisive = {}


def decisive_cases(V, T):
    """[(z, top_p, n_star)] for every intended size of n_stars(V); built once."""
    if (V, T) not in _decisive:
        rng = np.random.default_rng([V, int(T * 10), 17])
        _decisive[(V, T)] = [decisive_row(V, T, n, rng) for n in n_stars(V)]
    return _decisive[(V, T)]


def decisive_host_draws(V, T):
    """Per case of decisive_cases(V, T): (host tokens [S], excused [S]) at step current = 1 with DECISIVE_SEED."""
    return [check_draws([z] * DECISIVE_S, DECISIVE_S, T, 0, top_p, DECISIVE_SEED, 1) for z, top_p, _ in decisive_cases(V, T)]


# ------------------------------------------------------------------------------------------------ the production-shape fixture (bf16)
PROD_E = PROD_H = 1000
PROD_V = 10640
PROD_N, PROD_S = 1024, 5      # 5120 rows
PROD_WOUT = 1500.0            # see production_model


def production_model(seed=4):
    """The decisive model of tests/test_gpu_sample.py with Wout scaled further (PROD_WOUT instead of 8; measured with the oracle: 600 judges 28 of the 47 sampled rows, 1500 all, lowest share 0.15): at 8 the distribution is the
    bias's and the top word holds under 2 %; the structural bf16 test needs rows whose top word holds >= 10 % at every step."""
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    m = orc.init_weights(PROD_E, PROD_H, PROD_H, PROD_V, seed=seed)
    for n in ("W1", "W2", "Wout"):
        m.p[n] *= 2.0
    m.p["Wout"][:] *= PROD_WOUT
    m.p["bout"][:] = (rng.standard_normal((1, PROD_V)) * 2.0).astype(np.float32)
    m.p["b1"][:] += (rng.standard_normal(m.p["b1"].shape) * 0.5).astype(np.float32)
    return m


def production_feats(seed=11):
    return (np.random.default_rng(seed).standard_normal((PROD_N, 4096)) * 0.05).astype(np.float32)


def production_rows():
    """The sample of rows that test_replay_production_bf16 replays."""
    R = PROD_N * PROD_S
    return sorted(set([0, 1, 2, 3, 4, 255, 256, 1279, 2560, 2561, 4095, R - 6, R - 2, R - 1] + list(range(7, R, 157))))


def judged(m, feats_rows, captions):
    """Per row: does the bf16-emulating oracle give the top word a share >= 0.1 at every step of the caption (token ids incl. bos, teacher
    forced)?"""
    from oracle import oracle as orc
    Tn = max(len(c) for c in captions) - 1
    toks = np.zeros((max(Tn, 1), len(captions)), np.int32)
    for b, seq in enumerate(captions):
        for t in range(len(seq) - 2):
            toks[t, b] = seq[t + 1]
    with orc.emulate_bf16():
        z_all = orc.forward_logits(m, feats_rows, toks).astype(np.float64)
    out = []
    for b, seq in enumerate(captions):
        ok = True
        for t in range(len(seq) - 1):
            z = z_all[t, b]
            p = np.exp(z - z.max())
            ok = ok and p.max() / p.sum() >= 0.1
        out.append(ok)
    return np.array(out)


def oracle_greedy(m, feats_rows, nword):
    """Greedy captions (token ids incl. bos) of the bf16-emulating oracle, teacher forcing its own choices step by step."""
    from oracle import oracle as orc
    B = feats_rows.shape[0]
    seqs = [[1] for _ in range(B)]
    for t in range(nword + 1):
        toks = np.zeros((max(t, 1), B), np.int32)
        for b, s in enumerate(seqs):
            for u in range(min(t, len(s) - 1)):
                toks[u, b] = s[u + 1]
        with orc.emulate_bf16():
            z = orc.forward_logits(m, feats_rows, toks[:max(t, 1)])[t]
        for b, s in enumerate(seqs):
            if len(s) == t + 1 and (t == 0 or s[-1] != 0):
                s.append(int(np.argmax(z[b])))
    return seqs
