"""The weighted caption loss and gradient of include/lrcn_weighted.h from the CPU oracle (tests only): tests/varlen_ref.py generalised,
nothing of the code under test.

    loss = -(1 / norm_tokens) * sum_b w[b] * sum_{s <= len_b} log p_{s,b}[y_{s,b}]

Row b is a one-row batch of the equal-length oracle, orc.loss(..., norm_B = n_b) = -(1 / (n_b (len_b + 1))) sum_s log p, which enters with
the combination weight n_b (len_b + 1) / norm_tokens (varlen_ref) times w[b]; a negative weight negates the row's float64 gradient, a zero
one leaves the row out.  Under orc.emulate_bf16() the oracle rounds d(logits) after scaling it by 1 / (n_b (len_b + 1)): with
n_b = norm_tokens / (|w[b]| (len_b + 1)) -- an integer for the weights and lengths of bf16_case() -- that is the library's scale
|w[b]| / norm_tokens exactly, the combination weight is sign(w[b]), and bf16 rounding is symmetric in the sign.
"""
import numpy as np

from oracle import oracle as orc

import varlen_ref as vr

POW2_WEIGHTS = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)


def integer_row_norms(lens, weights, norm_tokens):
    """n_b = norm_tokens / (|w_b| (len_b + 1)) for every row with a weight, 1 for a zero-weight row; asserts each is an integer."""
    out = []
    for n, w in zip(lens, weights):
        if w == 0:
            out.append(1)
            continue
        q = norm_tokens / (abs(float(w)) * (int(n) + 1))
        assert q == int(q) and q >= 1, "norm_tokens %d / (|%g| * %d) is not an integer" % (norm_tokens, w, int(n) + 1)
        out.append(int(q))
    return out


def loss(model, feats, tokens, lens, weights, norm_tokens=None, mask1=None, mask2=None, want_grad=False, row_norms=None, fast=False):
    """tokens [Tmax][B] (entries at t >= lens[b], and all of a zero-weight row, are never looked at), lens [B], weights [B] (read as the
    float32 values the library receives), masks (Tmax + 1, B, .) as orc.loss takes them."""
    tokens = np.asarray(tokens, dtype=np.int32)
    feats = np.asarray(feats, dtype=np.float32)
    weights = np.asarray(weights, dtype=np.float32).astype(np.float64)
    B = len(lens)
    assert weights.shape == (B,)
    nt = vr.norm_tokens_of(lens) if norm_tokens is None else int(norm_tokens)
    total = 0.0
    acc = {k: np.zeros(np.asarray(model.p[k]).shape, np.float64) for k in orc.PARAM_NAMES} if want_grad else None
    for b in range(B):
        if weights[b] == 0.0:
            continue
        n = int(lens[b])
        nb = 1 if row_norms is None else int(row_norms[b])
        w = weights[b] * nb * (n + 1) / nt
        kw = {}
        if mask1 is not None:
            kw["mask1"] = np.asarray(mask1)[:n + 1, b:b + 1]
        if mask2 is not None:
            kw["mask2"] = np.asarray(mask2)[:n + 1, b:b + 1]
        r = orc.loss(model, feats[b:b + 1], tokens[:n, b:b + 1].reshape(n, 1), norm_B=nb, want_grad=want_grad, fast=fast, **kw)
        val, g = r if want_grad else (r, None)
        total += w * float(val)
        if want_grad:
            for k in orc.PARAM_NAMES:
                acc[k] += w * g.p[k].astype(np.float64)
    return (total, vr.Grads(acc)) if want_grad else total


def emulated_reference(model, feats, tokens, lens, weights, norm_tokens, **kw):
    """As varlen_ref.emulated_reference: (loss, gradients) under bf16 emulation with d(logits) rounded at the library's scale, `.f32` = the
    same from the plain oracle."""
    nb = integer_row_norms(lens, weights, norm_tokens)
    with orc.emulate_bf16():
        e_loss, e_g = loss(model, feats, tokens, lens, weights, norm_tokens, want_grad=True, row_norms=nb, **kw)
    e_g.f32 = loss(model, feats, tokens, lens, weights, norm_tokens, want_grad=True, **kw)
    return e_loss, e_g


def bf16_case(B, rng):
    """(lens, weights, norm_tokens) for the bf16-emulating form: lengths with integer shares, weights that are powers of two of either sign
    (scale * w is exact in f32), norm_tokens four times the batch's own count -- every row's n_b is then an integer."""
    lens = vr.lens_with_integer_shares(B, rng)
    weights = rng.choice(POW2_WEIGHTS, size=B).astype(np.float32)
    nt = 4 * vr.norm_tokens_of(lens)
    integer_row_norms(lens, weights, nt)
    return lens, weights, nt


class WeightedOracleOps(vr.VarlenOracleOps):
    """CPU stand-in of dp.HipOps whose lossgradient takes row_weights (the gloo test)."""

    def lossgradient(self, param, feats, tokens, norm_B, pdrop, seed, grads, lens=None, norm_tokens=None, row_weights=None):
        import torch
        if row_weights is None:
            return vr.VarlenOracleOps.lossgradient(self, param, feats, tokens, norm_B, pdrop, seed, grads, lens=lens, norm_tokens=norm_tokens)
        val, g = loss(self.base._model(param), feats.numpy(), tokens, lens, row_weights, norm_tokens, want_grad=True)
        self.base._loss = val
        for n, t in zip(orc.PARAM_NAMES, grads):
            t.copy_(torch.as_tensor(g.p[n].astype(np.float32)))
