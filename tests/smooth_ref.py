"""Host restatement of label smoothing (include/lrcn_smooth.h), tests only, in float64: the cross-entropy stage on given logits rows
(numpy, the header's formulas as written) and the caption model on tests/torch_ref.py's lrcn / lrcn1 steps as tests/sched_ref.py builds
it -- lens, row weights, masks, fed inputs -- with autograd for the gradients.  Nothing here comes from the HIP sources."""
import numpy as np
import torch

import sched_ref as sr
from oracle import oracle as orc

EOS = 0
F64 = torch.float64


def xent_rows(logits, tgt, eps, row_w=None, B=None, scale=1.0):
    """logits (M, V), tgt (M) -> (terms, ll_terms, dlog) in float64.  Row m carries w = row_w[m % B] (1 without row_w); a target outside
    [0, V) or a weight 0 makes it inactive: terms 0, a zero dlog row, logits not looked at (they may be NaN).
      ll = (z_t - max) - log se,  u = mean(z - max) - log se,  term = w ((1 - eps) ll + eps u),  dlog = (softmax - q) scale w."""
    z = np.asarray(logits, np.float64)
    tgt = np.asarray(tgt)
    M, V = z.shape
    B = M if B is None else B
    terms, ll_terms, dlog = np.zeros(M), np.zeros(M), np.zeros((M, V))
    for m in range(M):
        w = 1.0 if row_w is None else float(np.float32(row_w[m % B]))
        t = int(tgt[m])
        if t < 0 or t >= V or w == 0.0:
            continue
        d = z[m] - z[m].max()
        lse = np.log(np.exp(d).sum())
        ll, u = d[t] - lse, d.mean() - lse
        terms[m] = w * ((1.0 - eps) * ll + eps * u)
        ll_terms[m] = w * ll
        q = np.full(V, eps / V)
        q[t] += 1.0 - eps
        dlog[m] = (np.exp(d - lse) - q) * (scale * w)
    return terms, ll_terms, dlog


def loss(model, feats, tokens, lens, eps, fed=None, norm_tokens=None, row_w=None, mask1=None, mask2=None, want_grad=False):
    """The smoothed caption loss -(1 / norm_tokens) sum_b w_b sum_{s <= lens[b]} ((1 - eps) log p[gold] + eps mean_v log p[v]) with the step
    inputs fed[s] (default: the gold inputs of the padded batch).  -> (loss, nll), or (loss, nll, Grads) with want_grad; nll is the same sum
    with eps = 0."""
    tokens, lens = np.asarray(tokens), np.asarray(lens)
    T, B = tokens.shape
    fed = sr.gold_inputs(tokens, lens) if fed is None else np.asarray(fed)
    p = sr._params(model, want_grad)
    step, state = sr._stepper(p)
    s = [torch.zeros(B, H, dtype=F64) for H in state]
    x_cnn = torch.as_tensor(np.asarray(feats), dtype=F64) @ p["Wcnn"]
    w = torch.ones(B, dtype=F64) if row_w is None else torch.as_tensor(np.asarray(row_w, np.float32), dtype=F64)
    ln = torch.as_tensor(lens, dtype=torch.long)
    total, plain = 0.0, 0.0
    for t in range(T + 1):
        y = step(p, s, x_cnn, p["Wembed"][torch.as_tensor(fed[t], dtype=torch.long)], sr._m(mask1, t), sr._m(mask2, t))
        tgt = torch.as_tensor(tokens[t] if t < T else np.zeros(B), dtype=torch.long)
        tgt = torch.where(t < ln, tgt, torch.full_like(tgt, EOS))
        lp = torch.log_softmax(y, 1)
        act = (t <= ln).to(F64) * w
        ll = lp[torch.arange(B), tgt]
        total = total + (((1.0 - eps) * ll + eps * lp.mean(1)) * act).sum()
        plain = plain + float((ll.detach() * act).sum())
    nt = int(lens.astype(np.int64).sum()) + B if norm_tokens is None else int(norm_tokens)
    val = -total / nt
    if not want_grad:
        return float(val), -plain / nt
    val.backward()
    g = {n: (p[n].grad.numpy() if n in p and p[n].grad is not None else np.zeros(np.asarray(model.p[n]).shape)) for n in orc.PARAM_NAMES}
    return float(val.detach()), -plain / nt, sr.Grads(g)
