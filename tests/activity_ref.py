"""torch-CPU float64 restatement of the activity model of include/lrcn_activity.h (tests only).

  reference(...)  forward, loss, autograd gradients and clip / frame probabilities in float64 -- nothing taken from the HIP sources
  emulated(...)   the same model with a hand-written backward pass, rounded to bfloat16 exactly where the header says the bf16 path stores
                  or feeds bf16 (bf16=False: no rounding; the tests hold it against reference() so the hand-written backward is checked too)

Arrays are numpy in the ABI's logical shapes: W (F+H) x 4H, b 1 x 4H, Wout H x C, bout 1 x C, feats (B*T) x F with row b*T + t.
Returns (loss, [dW, db, dWout, dbout], clip_probs C x B, frame_probs C x (B*T)).
"""
import numpy as np
import torch


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _mask(lens, T, B):
    lens = np.full(B, T, np.int64) if lens is None else np.asarray(lens, np.int64)
    m = torch.zeros(T, B, dtype=torch.float64)
    for b in range(B):
        m[:int(lens[b]), b] = 1.0
    return m, lens


def _outputs(p, m, lens, T, B):
    C = p.shape[-1]
    clip = (p * m[:, :, None]).sum(0) / torch.as_tensor(lens, dtype=torch.float64)[:, None]   # B x C
    frame = (p * m[:, :, None]).permute(1, 0, 2).reshape(B * T, C)                            # (b*T + t) x C
    return clip.T.numpy().copy(), frame.T.numpy().copy()


def reference(W, b, Wout, bout, feats, labels, lens, T, B):
    F = feats.shape[1]
    H = Wout.shape[0]
    params = [_t(x).requires_grad_(True) for x in (W, b, Wout, bout)]
    W_, b_, Wo, bo = params
    x = _t(feats).reshape(B, T, F)
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    zs = []
    for t in range(T):
        g = torch.cat([x[:, t], h], 1) @ W_ + b_
        f, i, o, gg = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.sigmoid(g[:, 2 * H:3 * H]), torch.tanh(g[:, 3 * H:])
        c = c * f + i * gg
        h = o * torch.tanh(c)
        zs.append(h @ Wo + bo)
    z = torch.stack(zs)                                   # T x B x C
    logp = torch.log_softmax(z, -1)
    m, lens = _mask(lens, T, B)
    loss = None
    grads = None
    if labels is not None:
        lab = torch.as_tensor(np.asarray(labels, np.int64))
        pick = logp.gather(2, lab[None, :, None].expand(T, B, 1))[:, :, 0]
        loss = -(pick * m).sum() / float(lens.sum())
        loss.backward()
        grads = [q.grad.numpy().copy() for q in params]
        loss = float(loss.detach())
    clip, frame = _outputs(logp.detach().exp(), m, lens, T, B)
    return loss, grads, clip, frame


def _bf16(a):
    return a.to(torch.bfloat16).to(torch.float64)


def emulated(W, b, Wout, bout, feats, labels, lens, T, B, bf16=True):
    r = _bf16 if bf16 else (lambda a: a)
    F = feats.shape[1]
    H, C = Wout.shape
    W_, b_, Wo_, bo = _t(W), _t(b), _t(Wout), _t(bout)
    Wx, Wh, Wo = r(W_[:F]), r(W_[F:]), r(Wo_)
    x = r(_t(feats).reshape(B, T, F))
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    hs, cs, acts = [], [], []
    for t in range(T):
        g = x[:, t] @ Wx + b_ + h @ Wh                    # h: the stored (rounded) copy
        f, i, o, gg = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.sigmoid(g[:, 2 * H:3 * H]), torch.tanh(g[:, 3 * H:])
        c = c * f + i * gg                                # f32 cell from the unrounded gates
        h = r(o * torch.tanh(c))
        acts.append([r(f), r(i), r(o), r(gg)])            # what the backward pass reads
        hs.append(h)
        cs.append(c)
    Hs = torch.stack(hs)                                  # T x B x H
    z = Hs @ Wo + bo
    logp = torch.log_softmax(z, -1)
    p = logp.exp()
    m, lens = _mask(lens, T, B)
    clip, frame = _outputs(p, m, lens, T, B)
    if labels is None:
        return None, None, clip, frame
    lab = torch.as_tensor(np.asarray(labels, np.int64))
    tot = float(lens.sum())
    pick = logp.gather(2, lab[None, :, None].expand(T, B, 1))[:, :, 0]
    loss = float(-(pick * m).sum() / tot)
    onehot = torch.zeros(T, B, C, dtype=torch.float64)
    onehot[:, torch.arange(B), lab] = 1.0
    dlog = r((p - onehot) * (1.0 / tot) * m[:, :, None])
    dWo = torch.einsum("tbh,tbc->hc", Hs, dlog)
    dbo = dlog.sum((0, 1))[None, :]
    dh_ext = dlog @ Wo.T                                  # T x B x H
    dZ = [None] * T
    dc = torch.zeros(B, H, dtype=torch.float64)
    dhrec = torch.zeros(B, H, dtype=torch.float64)
    WhT = r(W_[F:]).T                                     # 4H x H
    for t in range(T - 1, -1, -1):
        f, i, o, gg = acts[t]
        dh = dh_ext[t] + dhrec
        tc = torch.tanh(cs[t])
        do = dh * tc
        dcv = dc + dh * o * (1.0 - tc * tc)
        cp = cs[t - 1] if t > 0 else torch.zeros_like(dc)
        z_ = torch.cat([dcv * cp * f * (1 - f), dcv * gg * i * (1 - i), do * o * (1 - o), dcv * i * (1 - gg * gg)], 1)
        dZ[t] = r(z_)
        dc = dcv * f
        dhrec = dZ[t] @ WhT
    dZs = torch.stack(dZ)                                 # T x B x 4H
    hprev = torch.cat([torch.zeros(1, B, H, dtype=torch.float64), Hs[:-1]], 0)
    dW = torch.cat([torch.einsum("tbf,tbg->fg", x.permute(1, 0, 2), dZs), torch.einsum("tbh,tbg->hg", hprev, dZs)], 0)
    db = dZs.sum((0, 1))[None, :]
    return loss, [dW.numpy(), db.numpy(), dWo.numpy(), dbo.numpy()], clip, frame


def order_task(n, T, F, seed, pattern_seed=0):
    """The synthetic order task: every clip shows pattern A at one step and pattern B at another (plus noise), class 0 if A comes first,
    class 1 otherwise.  The set of frames is the same for both classes, so no per-frame classifier beats chance.  The two patterns
    depend on pattern_seed only; the clips on seed."""
    prng = np.random.default_rng(pattern_seed)
    pa = prng.standard_normal(F)
    pb = prng.standard_normal(F)
    rng = np.random.default_rng(seed)
    feats = 0.3 * rng.standard_normal((n * T, F))
    labels = rng.integers(0, 2, n).astype(np.int32)
    for k in range(n):
        t1, t2 = sorted(rng.choice(T, 2, replace=False))
        first, second = (pa, pb) if labels[k] == 0 else (pb, pa)
        feats[k * T + t1] += first
        feats[k * T + t2] += second
    return feats.astype(np.float32), labels
