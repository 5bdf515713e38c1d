"""The masked caption loss and gradient of include/lrcn_varlen.h from the CPU oracle (tests only): the per-caption sums of the EXISTING
equal-length oracle, nothing of the code under test.

Row b of a padded batch is a one-row batch of length len_b:  orc.loss(model, feats[b], tokens[:len_b, b], norm_B = n_b)
    = -(1 / (n_b (len_b + 1))) * sum_{s <= len_b} log p_{s,b}[y_{s,b}],
so the masked loss  -(1 / norm_tokens) * sum_b sum_s log p  is the sum of the rows' values with weights n_b (len_b + 1) / norm_tokens, and
the gradient the same combination of the rows' gradients (float64 sums).  n_b is free: 1 by default.  Under orc.emulate_bf16() the
oracle rounds d(logits) after scaling it by 1 / (n_b (len_b + 1)); with n_b = norm_tokens / (len_b + 1) (an integer, the caller's choice of
lengths) that is the library's scale 1 / norm_tokens exactly and the weight is 1.
"""
import numpy as np

from oracle import oracle as orc


def norm_tokens_of(lens):
    return int(np.asarray(lens, dtype=np.int64).sum()) + len(lens)


def integer_row_norms(lens, norm_tokens=None):
    """n_b = norm_tokens / (len_b + 1) for every row, or None when one of them is not an integer."""
    nt = norm_tokens_of(lens) if norm_tokens is None else int(norm_tokens)
    if any(nt % (int(n) + 1) for n in lens):
        return None
    return [nt // (int(n) + 1) for n in lens]


class Grads:
    """float64 gradients by tensor name, like the oracle's gradient Model (`.p`)."""

    def __init__(self, p):
        self.p = p
        self.f32 = None


def loss(model, feats, tokens, lens, norm_tokens=None, mask1=None, mask2=None, want_grad=False, row_norms=None, fast=False):
    """tokens [Tmax][B] (entries at t >= lens[b] are never looked at), lens [B], masks (Tmax + 1, B, .) as orc.loss takes them."""
    tokens = np.asarray(tokens, dtype=np.int32)
    feats = np.asarray(feats, dtype=np.float32)
    B = len(lens)
    nt = norm_tokens_of(lens) if norm_tokens is None else int(norm_tokens)
    total, acc = 0.0, None
    for b in range(B):
        n = int(lens[b])
        nb = 1 if row_norms is None else int(row_norms[b])
        w = nb * (n + 1) / nt
        kw = {}
        if mask1 is not None:
            kw["mask1"] = np.asarray(mask1)[:n + 1, b:b + 1]
        if mask2 is not None:
            kw["mask2"] = np.asarray(mask2)[:n + 1, b:b + 1]
        r = orc.loss(model, feats[b:b + 1], tokens[:n, b:b + 1].reshape(n, 1), norm_B=nb, want_grad=want_grad, fast=fast, **kw)
        val, g = r if want_grad else (r, None)
        total += w * float(val)
        if want_grad:
            if acc is None:
                acc = {k: np.zeros(g.p[k].shape, np.float64) for k in orc.PARAM_NAMES}
            for k in orc.PARAM_NAMES:
                acc[k] += w * g.p[k].astype(np.float64)
    return (total, Grads(acc)) if want_grad else total


def emulated_reference(model, feats, tokens, lens, norm_tokens=None, row_norms=None, **kw):
    """As parity_util.emulated_reference: (loss, gradients) under bf16 emulation, `.f32` = the same from the plain oracle."""
    with orc.emulate_bf16():
        e_loss, e_g = loss(model, feats, tokens, lens, norm_tokens, want_grad=True, row_norms=row_norms, **kw)
    e_g.f32 = loss(model, feats, tokens, lens, norm_tokens, want_grad=True, **kw)
    return e_loss, e_g


def pad_with(tokens, lens, fill):
    """A copy of tokens [Tmax][B] whose entries past each row's length are taken from `fill` (scalar or array)."""
    t = np.array(tokens, dtype=np.int32)
    f = np.broadcast_to(np.asarray(fill, dtype=np.int32), t.shape)
    for b, n in enumerate(lens):
        t[int(n):, b] = f[int(n):, b]
    return t


def lens_with_integer_shares(B, rng, choices=(0, 1, 2, 3, 5)):
    """B lengths drawn from `choices` such that sum(lens + 1) is a multiple of every len + 1 (the last three rows are chosen for that)."""
    import itertools
    import math
    lcm = 1
    for c in choices:
        lcm = lcm * (c + 1) // math.gcd(lcm, c + 1)
    lens = [int(c) for c in rng.choice(choices, size=B)]
    for tail in itertools.product(choices, repeat=3):
        cand = lens[:-3] + list(tail)
        if norm_tokens_of(cand) % lcm == 0:
            return np.asarray(cand, dtype=np.int32)
    raise AssertionError("no such tail")


class VarlenOracleOps:
    """CPU stand-in of dp.HipOps for padded batches (the gloo test): lossgradient / loss from this module, the rest as
    tests/dp_oracle_ops.py."""

    def __init__(self, base):
        self.base = base

    def __getattr__(self, name):
        return getattr(self.base, name)

    def lossgradient(self, param, feats, tokens, norm_B, pdrop, seed, grads, lens=None, norm_tokens=None):
        import torch
        if lens is None:
            return self.base.lossgradient(param, feats, tokens, norm_B, pdrop, seed, grads)
        val, g = loss(self.base._model(param), feats.numpy(), tokens, lens, norm_tokens, want_grad=True)
        self.base._loss = val
        for n, t in zip(orc.PARAM_NAMES, grads):
            t.copy_(torch.as_tensor(g.p[n].astype(np.float32)))

    def loss(self, param, feats, tokens, lens=None):
        if lens is None:
            return self.base.loss(param, feats, tokens)
        return loss(self.base._model(param), feats.numpy(), tokens, lens)
