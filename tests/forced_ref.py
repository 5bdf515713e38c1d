"""Host restatement of forced-word beam search (include/lrcn_forced.h, lrcn_beam_forced_batch), rule for rule, in float32: the search of
tests/constrained_ref.py with one bank of K slots per state of the forced-word automaton and one pool per image.  The helpers of
nbest_ref.py (log_softmax, pool_insert, length_factor) and constrained_ref.py (topk_allowed, the `allowed` hook) are imported, not restated.

An image's sets are a list of up to 3 lists of alternative token ids; an id < 0 is no word and a set without ids is absent.  The position
(c, a) of a word in that list is its place in the candidate order.
"""
import numpy as np

import constrained_ref as cr
import nbest_ref as nb

EOS, BOS = nb.EOS, nb.BOS


def full_of(sets):
    """the mask of the present sets"""
    return sum(1 << c for c, alt in enumerate(sets) if any(w >= 0 for w in alt))


def state_of(history, sets):
    """history: tokens, bos first.  -> the mask whose bit c is set iff some word after bos is in set c"""
    words = set(int(t) for t in history[1:])
    return sum(1 << c for c, alt in enumerate(sets) if any(w >= 0 and int(w) in words for w in alt))


def meets(tokens, sets):
    """Does an entry (tokens incl. bos) hold a word of every present set?"""
    return state_of(tokens, sets) == full_of(sets)


def proposals(lp, K, history, current, sets, ban=()):
    """One live row: lp its log-softmax over all V columns, ban the columns rules 1-3 do not allow.
    -> (stay columns [K], their logp [K], moves [(c, a, word, logp)] in (c, a) order)."""
    assert len(history) == current
    b, full = state_of(history, sets), full_of(sets)
    ban = set(int(v) for v in ban)
    unmet = [(c, a, int(w)) for c, alt in enumerate(sets) for a, w in enumerate(alt) if w >= 0 and not (b >> c) & 1]
    moves = [(c, a, w, np.float32(lp[w])) for c, a, w in unmet if w not in ban and lp[w] > -np.inf]
    stay_ban = ban | set(w for _, _, w in unmet)
    if b != full:
        stay_ban.add(EOS)   # rule 4
    cols, vals = cr.topk_allowed(lp, K, stay_ban)
    return cols, vals, moves


def search_forced(step, N, K, nword, alpha, forced, allowed=None, early_stop=True):
    """forced: per image its list of sets.  -> per image the pool [(tokens incl. bos, logp, score)], best first."""
    assert len(forced) == N
    allowed = allowed or (lambda history, current: ())
    live = [{0: [([BOS], np.float32(0.0), None)]} for _ in range(N)]   # bank -> [(history, cum, handle)]; step 1: row 0 of bank 0 alone
    pools = [[] for _ in range(N)]
    done = [False] * N
    lpmax = nb.length_factor(nword + 1, alpha)
    for current in range(1, nword + 2):
        req, owner = [], []
        for n in range(N):
            if done[n]:
                continue
            for b in sorted(live[n]):
                for i, (hist, _, h) in enumerate(live[n][b]):
                    req.append((n, h, hist[-1]))
                    owner.append((n, b, i))
        if not req:
            break
        logits, handles = step(req)
        props = {}
        for q, (n, b, i) in enumerate(owner):
            hist = live[n][b][i][0]
            assert state_of(hist, forced[n]) == b
            props[(n, b, i)] = proposals(nb.log_softmax(logits[q]), K, hist, current, forced[n], allowed(hist, current)) + (handles[q],)
        lpc = nb.length_factor(current, alpha)
        for n in range(N):
            if done[n]:
                continue
            sets, full = forced[n], full_of(forced[n])
            new = {}
            for bt in range(1 << len(sets)):
                if bt & ~full:
                    continue
                cands = []   # (value, candidate order, history, word, handle)
                for i, (hist, cum, _) in enumerate(live[n].get(bt, [])):
                    cols, vals, _, h = props[(n, bt, i)]
                    for j in range(K):
                        cands.append((np.float32(cum + vals[j]), (bt * K + i, 0, j, 0), hist, int(cols[j]), h))
                for c in range(len(sets)):
                    if not (bt >> c) & 1:
                        continue
                    src = bt ^ (1 << c)
                    for i, (hist, cum, _) in enumerate(live[n].get(src, [])):
                        _, _, moves, h = props[(n, src, i)]
                        for cc, a, w, v in moves:
                            if cc == c:
                                cands.append((np.float32(cum + v), (src * K + i, 1, c, a), hist, w, h))
                cands.sort(key=lambda t: (-float(t[0]), t[1]))
                slots = []
                for v, _, hist, tok, h in cands:
                    if tok == EOS:
                        assert bt == full
                        nb.pool_insert(pools[n], K, (hist + [EOS], v, np.float32(v / lpc)))
                    else:
                        slots.append((hist + [tok], v, h))
                        if len(slots) == K:
                            break
                if slots:
                    new[bt] = slots
            alive = [c for s in new.values() for _, c, _ in s]
            if current == nword + 1:
                for hist, v, _ in new.get(full, []):
                    nb.pool_insert(pools[n], K, (hist, v, np.float32(v / lpc)))
                done[n] = True
            elif not alive:
                done[n] = True
            elif early_stop and len(pools[n]) == K and pools[n][-1][2] >= np.float32(max(alive) / lpmax):
                done[n] = True
            live[n] = new
    return pools


# ---- what tests/test_forced_host.py and tests/test_gpu_forced.py share: the end-to-end cases on test_gpu_nbest.small_model ----
E2E_N, E2E_NWORD, E2E_FEAT_SEED = 8, 12, 7
E2E_CASES = [(1, 5), (2, 4), (3, 4)]   # (C, K): 2^C * K <= 32 rows per image
# Words that no constrained n-best list of the small models (either depth, K = 4 or 5, alpha 0 or 1, feature seed 7) holds, so every image
# with a set has to change its lists; two alternatives, one, and LRCN_FORCED_MAXALT of them.
E2E_SETS = [[56, 137], [50], [54, 26, 142, 181]]


def e2e_forced(C):
    """per image the first C sets; image 6 has none and image 7 a single set"""
    per = [[list(s) for s in E2E_SETS[:C]] for _ in range(E2E_N)]
    per[6] = []
    per[7] = [list(E2E_SETS[0])]
    return per


def perturbed(step, rel=1e-6):
    """`step` with every logit moved by a fixed relative pattern of +-rel (by column): what a different summation order may do to them"""
    def wrapped(req):
        z, handles = step(req)
        z = np.asarray(z, np.float32)
        sign = np.where((np.arange(z.shape[1]) * 7 + 3) % 5 < 2, 1.0, -1.0)
        return (z.astype(np.float64) * (1.0 + rel * sign)).astype(np.float32), handles
    return wrapped
