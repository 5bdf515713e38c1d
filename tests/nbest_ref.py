"""Host restatement of the n-best beam search of include/lrcn_nbest.h (lrcn_beam_nbest_batch), rule for rule, in float32.

`search(step, N, K, nword, alpha)` drives any source of logits through a callback:
    step(requests) -> (logits [len(requests)][V] float32, handles)
where requests[q] = (image, parent handle or None at step 1, input token); a handle names the row whose state a later request continues.
`table_step(V, seed)` makes seeded random logit tables (logits a function of image and history); `OracleStep` runs the CPU oracle's lrcn()
step per hypothesis with the states gathered by parent (under orc.emulate_bf16() for bf16 contexts).
"""
import math

import numpy as np

EOS, BOS = 0, 1


def log_softmax(z):
    """logp = (z - max z) - log(sum exp(z - max z)), float32 (the sum in float64)."""
    z = np.asarray(z, np.float32)
    d = (z - z.max()).astype(np.float32)
    se = np.float32(np.sum(np.exp(d.astype(np.float64))))
    return (d - np.float32(np.log(se))).astype(np.float32)


def length_factor(L, alpha):
    """lp(L) = (float)pow((double)L, alpha)"""
    return np.float32(math.pow(float(L), float(alpha)))


def topk(lp, K):
    """the K best columns by logp, descending, ties to the lower column"""
    order = np.lexsort((np.arange(len(lp)), -lp.astype(np.float64)))[:K]
    return order, lp[order]


def pool_insert(pool, K, entry):
    """entry = (tokens, logp, score): the K best scores, equal scores in insertion order, a full pool entered only by a strictly greater score"""
    sc = entry[2]
    if len(pool) == K:
        if not sc > pool[-1][2]:
            return
        pool.pop()
    q = len(pool)
    while q > 0 and pool[q - 1][2] < sc:
        q -= 1
    pool.insert(q, entry)


def search(step, N, K, nword, alpha, early_stop=True, trace=None):
    """-> per image the pool: [(tokens incl. bos, logp, score)], best first.  early_stop=False runs every image to nword+1.
    trace (a list) receives (image, step) for every step an image takes part in."""
    live = [[([BOS], np.float32(0.0), None)] for _ in range(N)]   # (history, cum, handle); step 1: slot 0 alone
    pools = [[] for _ in range(N)]
    done = [False] * N
    lpmax = length_factor(nword + 1, alpha)
    for current in range(1, nword + 2):
        req, owner = [], []
        for n in range(N):
            if done[n]:
                continue
            for i, (hist, _, h) in enumerate(live[n]):
                req.append((n, h, hist[-1]))
                owner.append((n, i))
            if trace is not None:
                trace.append((n, current))
        if not req:
            break
        logits, handles = step(req)
        props = {}
        for q, (n, i) in enumerate(owner):
            cols, vals = topk(log_softmax(logits[q]), K)
            props[(n, i)] = (cols, vals, handles[q])
        lpc = length_factor(current, alpha)
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
                    pool_insert(pools[n], K, (hist + [EOS], v, np.float32(v / lpc)))
                else:
                    new.append((hist + [tok], v, h))
                    if len(new) == K:
                        break
            if current == nword + 1:
                for hist, v, _ in new:
                    pool_insert(pools[n], K, (hist, v, np.float32(v / lpc)))
                done[n] = True
            elif not new:
                done[n] = True
            elif early_stop and len(pools[n]) == K and pools[n][-1][2] >= np.float32(max(c for _, c, _ in new) / lpmax):
                done[n] = True
            live[n] = new
    return pools


def greedy(step, N, nword):
    """argmax decoding (lowest column wins a tie) -> per image tokens incl. bos"""
    seqs = [[BOS] for _ in range(N)]
    handles = [None] * N
    active = list(range(N))
    for current in range(1, nword + 2):
        logits, hs = step([(n, handles[n], seqs[n][-1]) for n in active])
        nxt = []
        for q, n in enumerate(active):
            tok = int(np.argmax(log_softmax(logits[q])))
            seqs[n].append(tok)
            handles[n] = hs[q]
            if tok != EOS:
                nxt.append(n)
        active = nxt
        if not active:
            break
    return seqs


def table_step(V, seed, scale=3.0, quantum=None):
    """Seeded random logits as a function of (image, history); quantum rounds them to its multiples (ties).  Handles are the histories."""
    def step(req):
        out = np.zeros((len(req), V), np.float32)
        hs = []
        for q, (n, h, tok) in enumerate(req):
            hist = (h if h is not None else ()) + (int(tok),)
            rng = np.random.default_rng([seed, n] + list(hist))
            z = rng.standard_normal(V) * scale
            if quantum:
                z = np.round(z / quantum) * quantum
            out[q] = z.astype(np.float32)
            hs.append(hist)
        return out, hs
    return step


class OracleStep:
    """The CPU oracle's lrcn() step (lrcn.jl:540-551) for a set of hypotheses: x_cnn = feat * Wcnn per image, the embedding of the input
    token, and the states of the parent row (zero at step 1).  Handles are row indices into the previous call's states."""

    def __init__(self, orc, model, feats, bf16=False):
        self.orc, self.m, self.bf16 = orc, model, bf16
        f = np.asarray(feats, np.float32)
        W = model.p["Wcnn"]
        if bf16:
            f, W = orc.bf16_round(f), orc.bf16_round(W)
        self.xcnn = (f.astype(np.float64) @ np.asarray(W, np.float64)).astype(np.float32)
        self.prev = None

    def __call__(self, req):
        m, orc = self.m, self.orc
        B = len(req)
        Hs = [m.H1, m.H1, m.H2, m.H2] if m.n_layers == 2 else [m.H1, m.H1]
        if self.prev is None or all(h is None for _, h, _ in req):
            state = [np.zeros((B, H), np.float32, order="F") for H in Hs]
        else:
            rows = [h for _, h, _ in req]
            state = [np.asfortranarray(s[rows]) for s in self.prev]
        xc = np.stack([self.xcnn[n] for n, _, _ in req])
        emb = np.stack([m.p["Wembed"][tok] for _, _, tok in req]).astype(np.float32)
        if self.bf16:
            with orc.emulate_bf16():
                z = orc.lrcn_step(m, state, xc, emb)
        else:
            z = orc.lrcn_step(m, state, xc, emb)
        self.prev = [np.array(s) for s in state]
        return np.ascontiguousarray(z, np.float32), list(range(B))
