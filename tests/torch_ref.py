"""The torch-CPU *autograd* transcription of lrcn.jl: the second, independent statement of the caption model (tests only).

Forward only is transcribed; every gradient is torch autograd's, not hand-derived.  tests/golden/make_golden.py writes the committed golden
vectors with these functions, and the production-width tests (tests/production_width.py) call them at test time.  Nothing here comes from
oracle/ or from the HIP sources: it is a restatement of lrcn.jl alone, plus the per-row caption lengths of include/lrcn_varlen.h.

Every tensor this module creates carries an explicit dtype (float64 unless the caller passes another); it never touches torch's default
dtype, so importing it changes nothing for the other tests of the process.
"""
import numpy as np
import torch

EOS, BOS, UNK = 0, 1, 2
F64 = torch.float64


def lstm(W, b, h, c, x, gates=None):  # lrcn.jl:528-538
    g = torch.cat([x, h], 1) @ W + b
    if gates is not None:
        gates.append(g.detach())
    H = h.shape[1]
    f = torch.sigmoid(g[:, :H])
    i = torch.sigmoid(g[:, H:2 * H])
    o = torch.sigmoid(g[:, 2 * H:3 * H])
    gg = torch.tanh(g[:, 3 * H:])
    c = c * f + i * gg
    h = o * torch.tanh(c)
    return h, c


def lrcn(p, s, x_cnn, x_lstm, m1=None, m2=None, gates=None):  # lrcn.jl:540-551; gates: list that receives layer 1's pre-activations
    x = x_lstm if m1 is None else x_lstm * m1
    s[0], s[1] = lstm(p["W1"], p["b1"], s[0], s[1], x, gates)
    x = s[0] @ p["Wproj"]
    x = torch.cat([x, x_cnn], 1)
    if m2 is not None:
        x = x * m2
    s[2], s[3] = lstm(p["W2"], p["b2"], s[2], s[3], x)
    return s[2] @ p["Wout"] + p["bout"]


def lrcn1(p, s, x_cnn, x_lstm, m=None, m2=None, gates=None):  # LRCN-1f (oracle/lrcn_oracle.h states the definition); m2 is never set
    x = torch.cat([x_lstm, x_cnn], 1)
    if m is not None:
        x = x * m
    s[0], s[1] = lstm(p["W1"], p["b1"], s[0], s[1], x, gates)
    return s[0] @ p["Wout"] + p["bout"]


def _ids(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.long)


def _loss(step, state, p, feats, tokens, norm_B, mask1, mask2, collect, lens, norm_tokens, gates, dtype):
    """lrcn.jl:553-581 around `step` (lrcn or lrcn1).  lens (int [B]) / norm_tokens: the padded batch of include/lrcn_varlen.h -- row b is
    active at steps s <= lens[b], its target at s = lens[b] is eos, and the sum is divided by norm_tokens (default sum(lens + 1))."""
    T, B = tokens.shape
    s = [torch.zeros(B, H, dtype=dtype) for H in state]
    total = 0.0
    count = 0
    x_lstm = p["Wembed"][torch.full((B,), BOS, dtype=torch.long)]
    x_cnn = feats @ p["Wcnn"]
    ln = None if lens is None else _ids(lens)
    for t in range(T + 1):
        ypred = step(p, s, x_cnn, x_lstm, None if mask1 is None else mask1[t], None if mask2 is None else mask2[t], gates)
        if collect is not None:
            collect.append(ypred.detach())
        ynorm = torch.log_softmax(ypred, 1)
        tgt = _ids(tokens[t]) if t < T else torch.full((B,), EOS, dtype=torch.long)
        if ln is None:
            total = total + ynorm[torch.arange(B), tgt].sum()
            count += norm_B
        else:
            tgt = torch.where(t < ln, tgt, torch.full_like(tgt, EOS))      # eos at t = lens[b]; past it the row is inactive
            total = total + (ynorm[torch.arange(B), tgt] * (t <= ln).to(dtype)).sum()
        if t < T:
            x_lstm = p["Wembed"][tgt]
    if ln is not None:
        count = int(ln.sum()) + B if norm_tokens is None else int(norm_tokens)
    return -total / count


def loss(p, feats, tokens, norm_B, mask1=None, mask2=None, collect=None, lens=None, norm_tokens=None, gates=None, dtype=F64):
    H1, H2 = p["Wproj"].shape[0], p["Wout"].shape[0]
    return _loss(lrcn, (H1, H1, H2, H2), p, feats, tokens, norm_B, mask1, mask2, collect, lens, norm_tokens, gates, dtype)


def loss1(p, feats, tokens, norm_B, mask=None, collect=None, lens=None, norm_tokens=None, gates=None, dtype=F64):
    H = p["Wout"].shape[0]
    return _loss(lrcn1, (H, H), p, feats, tokens, norm_B, mask, None, collect, lens, norm_tokens, gates, dtype)


def adam_ref(w, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):  # Knet Adam defaults
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    w = w - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
    return w, m, v


def _beam(step, state, p, feat, K, nword, dtype):
    """lrcn.jl:585-678 / SURVEY A.3, float32 probabilities like the reference.  Returns the K final hypotheses, best first."""
    with torch.no_grad():
        x_cnn = feat @ p["Wcnn"]
        x = [([BOS], np.float32(1.0)) for _ in range(K)]
        states = [[torch.zeros(1, H, dtype=dtype) for H in state] for _ in range(K)]
        current = 1
        while True:
            new_x = []
            for i in range(K):
                last = x[i][0][-1]
                yp = step(p, states[i], x_cnn, p["Wembed"][last:last + 1])
                prob = torch.softmax(yp, 1).numpy().astype(np.float32).reshape(-1)
                top = np.argsort(-prob, kind="stable")[:K]
                for j in range(K):
                    new_x.append((x[i][0] + [int(top[j])], np.float32(prob[top[j]] * x[i][1])))
                if current == 1:
                    break
            order = np.argsort(-np.array([c[1] for c in new_x], np.float32), kind="stable")
            xs = [new_x[o] for o in order[:K]]
            if xs[0][0][-1] == EOS or current > nword:
                return xs
            states = [[t.clone() for t in states[order[i] // K]] for i in range(K)]
            x = xs
            current += 1


def beam_search_ref(p, feat, K, nword, dtype=F64):
    H1, H2 = p["Wproj"].shape[0], p["Wout"].shape[0]
    return _beam(lrcn, (H1, H1, H2, H2), p, feat, K, nword, dtype)


def beam_search_ref1(p, feat, K, nword, dtype=F64):
    H = p["Wout"].shape[0]
    return _beam(lrcn1, (H, H), p, feat, K, nword, dtype)
