"""Host restatement of constrained beam search (include/lrcn_constrain.h, lrcn_beam_constrained_batch), rule for rule, in float32: the
searches of tests/nbest_ref.py and tests/diverse_ref.py with one hook, `allowed(history, current) -> the columns that are NOT allowed`,
applied after nb.log_softmax and before the top-K.  Their helpers (log_softmax, topk, pool_insert, length_factor, penalised) are imported,
not restated; with a hook that bans nothing the searches below are those searches.

`banned_now(history, current, banned, min_len, n)` states the three rules; `hook(banned, min_len, n)` makes the search's hook from it.
"""
import numpy as np

import diverse_ref as dv
import nbest_ref as nb

EOS, BOS = nb.EOS, nb.BOS


def banned_now(history, current, banned, min_len, n):
    """history: the row's tokens, bos first, len(history) == current.  -> the set of columns that are not allowed at step `current`."""
    assert len(history) == current
    out = set(int(v) for v in banned)                                   # rule 1
    if current <= min_len:                                              # rule 2
        out.add(EOS)
    t = current - 1                                                     # rule 3: w_1 .. w_t = history[1 .. t]
    if n >= 1 and t >= n - 1:
        w = history
        suffix = list(w[t - n + 2:t + 1])
        for i in range(1, t - n + 2):
            if list(w[i:i + n - 1]) == suffix:
                out.add(int(w[i + n - 1]))
    return out


def hook(banned=(), min_len=0, n=0):
    return lambda history, current: banned_now(history, current, banned, min_len, n)


def topk_allowed(lp, K, ban):
    """the K best allowed columns by logp (of the whole row: nothing is renormalised), descending, ties to the lower column; columns of
    `ban` outside [0, V) are ignored"""
    m = np.array(lp, np.float32)
    cols = [v for v in ban if 0 <= v < len(m)]
    m[cols] = -np.inf
    order, vals = nb.topk(m, K)
    assert np.all(np.isfinite(vals)) or not np.all(np.isfinite(lp)), "fewer than K allowed columns"
    return order, vals


def search(step, N, K, nword, alpha, allowed=None, early_stop=True):
    """nbest_ref.search with the hook: per image the pool [(tokens incl. bos, logp, score)], best first."""
    allowed = allowed or (lambda history, current: ())
    live = [[([BOS], np.float32(0.0), None)] for _ in range(N)]
    pools = [[] for _ in range(N)]
    done = [False] * N
    lpmax = nb.length_factor(nword + 1, alpha)
    for current in range(1, nword + 2):
        req, owner = [], []
        for n in range(N):
            if done[n]:
                continue
            for i, (hist, _, h) in enumerate(live[n]):
                req.append((n, h, hist[-1]))
                owner.append((n, i))
        if not req:
            break
        logits, handles = step(req)
        props = {}
        for q, (n, i) in enumerate(owner):
            cols, vals = topk_allowed(nb.log_softmax(logits[q]), K, allowed(live[n][i][0], current))
            props[(n, i)] = (cols, vals, handles[q])
        lpc = nb.length_factor(current, alpha)
        for n in range(N):
            if done[n]:
                continue
            cands = []
            for i, (hist, cum, _) in enumerate(live[n]):
                cols, vals, h = props[(n, i)]
                for j in range(K):
                    cands.append((np.float32(cum + vals[j]), i * K + j, i, int(cols[j]), h))
            cands.sort(key=lambda t: (-float(t[0]), t[1]))
            new = []
            for v, _, i, tok, h in cands:
                hist = live[n][i][0]
                if tok == EOS:
                    nb.pool_insert(pools[n], K, (hist + [EOS], v, np.float32(v / lpc)))
                else:
                    new.append((hist + [tok], v, h))
                    if len(new) == K:
                        break
            if current == nword + 1:
                for hist, v, _ in new:
                    nb.pool_insert(pools[n], K, (hist, v, np.float32(v / lpc)))
                done[n] = True
            elif not new:
                done[n] = True
            elif early_stop and len(pools[n]) == K and pools[n][-1][2] >= np.float32(max(c for _, c, _ in new) / lpmax):
                done[n] = True
            live[n] = new
    return pools


def search_diverse(step, N, K, G, lam, nword, alpha, allowed=None, early_stop=True):
    """diverse_ref.search (its windowed form: the K best allowed columns, then the penalty) with the hook: per image a list of G pools."""
    assert G >= 1 and K % G == 0
    allowed = allowed or (lambda history, current: ())
    Kp = K // G
    live = [[[([BOS], np.float32(0.0), None)] for _ in range(G)] for _ in range(N)]
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
            cnt = {}
            settled = True
            for g in range(G):
                cands = []
                for i, (hist, cum, _) in enumerate(live[n][g]):
                    lp, h = rows[(n, g, i)]
                    cols, vals = topk_allowed(lp, K, allowed(hist, current))
                    for j, (w, a, v) in enumerate(dv.penalised(cols, vals, cnt, lam, Kp)):
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


def obeys(tokens, banned, min_len, n, nword):
    """Does a returned entry (tokens incl. bos; ends in eos unless truncated at nword + 1 words) obey the three rules?"""
    words = [t for t in tokens[1:] if t != EOS]
    ended = tokens[-1] == EOS
    if any(w in set(banned) for w in words):
        return False
    if ended and len(words) < min_len:
        return False
    if n >= 1:
        grams = [tuple(words[i:i + n]) for i in range(len(words) - n + 1)]
        if len(grams) != len(set(grams)):
            return False
    return ended or len(tokens) == nword + 2
