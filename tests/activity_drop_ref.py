"""torch-CPU float64 restatement of the activity model with dropout of include/lrcn_act_dropout.h (tests only; beside activity_ref.py).

  reference_drop(...)  the masked forward pass and its autograd gradients in float64 -- nothing taken from the HIP sources
  emulated_drop(...)   the hand-written backward of activity_ref.emulated with the two masks, rounded to bfloat16 where the header says the
                       bf16 path rounds (bf16=False: no rounding; the host tests hold it against reference_drop)

Arrays as in activity_ref; mask_in (T, B, F) and mask_out (T, B, H) are multiplier arrays in the logical shape (None: all ones), for a seeded
call dropout_ref.drop_mult(seed, 1, p_in, T, B, F) and drop_mult(seed, 2, p_out, T, B, H): seeded_masks().
Returns (loss, [dW, db, dWout, dbout]).
"""
import numpy as np
import torch

from activity_ref import _bf16, _mask, _t
from dropout_ref import drop_mult


def seeded_masks(seed, p_in, p_out, T, B, F, H):
    return drop_mult(seed, 1, p_in, T, B, F), drop_mult(seed, 2, p_out, T, B, H)


def _masks(mask_in, mask_out, T, B, F, H):
    mi = torch.ones(T, B, F, dtype=torch.float64) if mask_in is None else _t(mask_in)
    mo = torch.ones(T, B, H, dtype=torch.float64) if mask_out is None else _t(mask_out)
    assert tuple(mi.shape) == (T, B, F) and tuple(mo.shape) == (T, B, H)
    return mi, mo


def reference_drop(W, b, Wout, bout, feats, labels, lens, T, B, mask_in=None, mask_out=None):
    F = feats.shape[1]
    H = Wout.shape[0]
    params = [_t(x).requires_grad_(True) for x in (W, b, Wout, bout)]
    W_, b_, Wo, bo = params
    mi, mo = _masks(mask_in, mask_out, T, B, F, H)
    x = _t(feats).reshape(B, T, F) * mi.permute(1, 0, 2)
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    zs = []
    for t in range(T):
        g = torch.cat([x[:, t], h], 1) @ W_ + b_
        f, i, o, gg = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.sigmoid(g[:, 2 * H:3 * H]), torch.tanh(g[:, 3 * H:])
        c = c * f + i * gg
        h = o * torch.tanh(c)                              # the recurrent h: not masked
        zs.append((h * mo[t]) @ Wo + bo)
    logp = torch.log_softmax(torch.stack(zs), -1)          # T x B x C
    m, lens = _mask(lens, T, B)
    lab = torch.as_tensor(np.asarray(labels, np.int64))
    pick = logp.gather(2, lab[None, :, None].expand(T, B, 1))[:, :, 0]
    loss = -(pick * m).sum() / float(lens.sum())
    loss.backward()
    return float(loss.detach()), [q.grad.numpy().copy() for q in params]


def emulated_drop(W, b, Wout, bout, feats, labels, lens, T, B, mask_in=None, mask_out=None, bf16=True):
    r = _bf16 if bf16 else (lambda a: a)
    # the device forms the masked values as float32 products before it rounds them to bf16
    prod = (lambda a, m: (a.float() * m.float()).double()) if bf16 else (lambda a, m: a * m)
    F = feats.shape[1]
    H, C = Wout.shape
    W_, b_, Wo_, bo = _t(W), _t(b), _t(Wout), _t(bout)
    Wx, Wh, Wo = r(W_[:F]), r(W_[F:]), r(Wo_)
    mi, mo = _masks(mask_in, mask_out, T, B, F, H)
    x = r(prod(_t(feats).reshape(B, T, F), mi.permute(1, 0, 2)))   # X = bf16(feat * m_in): one rounding, after the product
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    hs, cs, acts = [], [], []
    for t in range(T):
        g = x[:, t] @ Wx + b_ + h @ Wh                    # h: the stored (rounded) unmasked copy
        f, i, o, gg = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.sigmoid(g[:, 2 * H:3 * H]), torch.tanh(g[:, 3 * H:])
        c = c * f + i * gg
        h = r(o * torch.tanh(c))
        acts.append([r(f), r(i), r(o), r(gg)])
        hs.append(h)
        cs.append(c)
    Hs = torch.stack(hs)                                  # T x B x H
    Hd = r(prod(Hs, mo))                                  # the head's operand: a second copy bf16(f32(h_bf16) * m_out)
    logp = torch.log_softmax(Hd @ Wo + bo, -1)
    p = logp.exp()
    m, lens = _mask(lens, T, B)
    lab = torch.as_tensor(np.asarray(labels, np.int64))
    tot = float(lens.sum())
    pick = logp.gather(2, lab[None, :, None].expand(T, B, 1))[:, :, 0]
    loss = float(-(pick * m).sum() / tot)
    onehot = torch.zeros(T, B, C, dtype=torch.float64)
    onehot[:, torch.arange(B), lab] = 1.0
    dlog = r((p - onehot) * (1.0 / tot) * m[:, :, None])
    dWo = torch.einsum("tbh,tbc->hc", Hd, dlog)           # dWout contracts Hd
    dbo = dlog.sum((0, 1))[None, :]
    dh_ext = (dlog @ Wo.T) * mo                           # dh = (dlog Wout') * m_out, not rounded
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
    hprev = torch.cat([torch.zeros(1, B, H, dtype=torch.float64), Hs[:-1]], 0)   # the unmasked h
    dW = torch.cat([torch.einsum("tbf,tbg->fg", x.permute(1, 0, 2), dZs), torch.einsum("tbh,tbg->hg", hprev, dZs)], 0)   # the masked X
    db = dZs.sum((0, 1))[None, :]
    return loss, [dW.numpy(), db.numpy(), dWo.numpy(), dbo.numpy()]
