"""Host restatement of diverse beam search (include/lrcn_diverse.h, lrcn_beam_diverse_batch), rule for rule, in float32.  It drives the
step callbacks of tests/nbest_ref.py (`table_step`, `OracleStep`) and reuses its log_softmax, topk, pool_insert and length_factor.

`search(step, N, K, G, lam, nword, alpha, early_stop=True, window=True)` -> per image a list of G pools, each [(tokens incl. bos, logp,
score)], best first.  early_stop=False runs every image to nword+1; window=False ranks all V penalised words of a row instead of the K best
unpenalised ones (the lemma of include/lrcn_diverse.h says the two agree).
"""
import numpy as np

import nbest_ref as nb

EOS, BOS = nb.EOS, nb.BOS


def penalised(cols, vals, cnt, lam, Kp):
    """a = fmaf(-lam, cnt(w), logp) over the given columns; the Kp best by (a descending, column ascending) -> [(word, a, logp)]"""
    c = np.array([cnt.get(int(w), 0) for w in cols], np.float64)
    # fmaf in float32: lam * cnt is exact in float64 (24 + 6 bits); the float64 sum then the float32 rounding differ from one rounding only
    # when the float64 sum lands on a float32 midpoint, which seeded inputs do not do.  cnt = 0 gives logp bit for bit.
    a =(np.float64(-np.float32(lam)) * c + np.asarray(vals, np.float64)).astype(np.float32)
    order = np.lexsort((np.asarray(cols), -a.astype(np.float64)))[:Kp]
    return [(int(cols[q]), a[q], np.float32(vals[q])) for q in order]


def search(step, N, K, G, lam, nword, alpha, early_stop=True, window=True):
    assert G >= 1 and K % G == 0
    Kp = K // G
    live = [[[([BOS], np.float32(0.0), None)] for _ in range(G)] for _ in range(N)]   # per group (history, cum, handle); step 1: slot 0 alone
    pools = [[[] for _ in range(G)] for _ in range(N)]
    done = [False] * N
    lpmax = nb.length_factor(nword + 1, alpha)
    for current in range(1, nword + 2):
        req, owner = [], []
        for n in range(N):
            if done[n]:
                continue
            for g in range(G):
                for i, (hist, _, h) in enumerate(live[n][g]):
                    req.append((n, h, hist[-1]))
                    owner.append((n, g, i))
        if not req:
            break
        logits, handles = step(req)
        rows = {own: (nb.log_softmax(logits[q]), handles[q]) for q, own in enumerate(owner)}
        lpc = nb.length_factor(current, alpha)
        for n in range(N):
            if done[n]:
                continue
            cnt = {}   # word -> live slots that earlier groups of this image filled with it at this step
            settled = True
            for g in range(G):
                cands = []
                for i, (hist, cum, _) in enumerate(live[n][g]):
                    lp, h = rows[(n, g, i)]
                    cols, vals = nb.topk(lp, K) if window else (np.arange(len(lp)), lp)
                    for j, (w, a, v) in enumerate(penalised(cols, vals, cnt, lam, Kp)):
                        cands.append((np.float32(cum + a), i * Kp + j, i, w, np.float32(cum + v), h))
                cands.sort(key=lambda t: (-float(t[0]), t[1]))
                new, pool = [], pools[n][g]
                for _, _, i, tok, v, h in cands:
                    hist = live[n][g][i][0]
                    if tok == EOS:
                        nb.pool_insert(pool, Kp, (hist + [EOS], v, np.float32(v / lpc)))
                    else:
                        new.append((hist + [tok], v, h))
                        if len(new) == Kp:
                            break
                for hist, _, _ in new:
                    cnt[hist[-1]] = cnt.get(hist[-1], 0) + 1
                if current == nword + 1:
                    for hist, v, _ in new:
                        nb.pool_insert(pool, Kp, (hist, v, np.float32(v / lpc)))
                satisfied = bool(new) and len(pool) == Kp and pool[-1][2] >= np.float32(max(c for _, c, _ in new) / lpmax)
                if new and not satisfied:
                    settled = False
                live[n][g] = new
            if current == nword + 1 or (early_stop and settled):
                done[n] = True
            elif all(not live[n][g] for g in range(G)):
                done[n] = True
    return pools
