"""GPU: the device-generated dropout mask (drop_mult / hash_uniform / mix64 of csrc/kernel_util.h, the default of train_step and of every
real run) against its host transcription (tests/dropout_ref.py).

The seeded mask is applied by two forward kernels (embed_gather, concat_x2) and four backward kernels (embed_scatter_rm, embed_segsum,
embed_rows_export, dx2_mask_reduce), each of which computes the counter (s, b, j) -> (s B + b) ncols + j on its own.  The route code of
train.hip never looks at the mask, so lossgradient(pdrop, seed) and lossgradient(mask1 = host, mask2 = host) are the same arithmetic with
the same multipliers -- if and only if every one of those kernels indexes the counter as the transcription does, uses stream 1 / 2 where it
does, compares u > p and multiplies by float32(1) / (float32(1) - float32(p)).  Under LRCN_OPT_DETERMINISTIC every sum has a fixed order,
so the demand is np.array_equal on the loss and on all nine gradients, in the two-layer model in f32 and bf16 and in LRCN-1f (one mask,
stream 1, over E + H/2 columns), at E = 72 / H = 64 / V = 301 / B = 6 / T = 5, at the same with B = 7 (T + 1 != B) and at E = H = 512 /
V = 2540; loss() likewise; and one train_step(pdrop, seed) equals lossgradient(masks) + update in parameters and both Adam moments.
Measured on an MI355X: bit-equal in every one of the sixteen runs (four draws, four models) and in the four train steps; nothing was loosened.
Deliberately wrong builds (never committed): stream 1 for the second mask fails every two-layer run and train step; `u >= p` fails the four
"edge" runs and, as it must, nothing at p = 0.4.  (b, s) swapped in embed_segsum's drop_mult passes "distinct" -- see SHAPES -- and is
caught by tests/test_gpu_embed_grad.py; "rows7" was added for it and not run on that build, whose explicit-mask branch would read past the mask.

The explicit-mask branch these runs are compared WITH is held to the CPU oracle and to float64 autograd by the parity tests; the seeded
branch is held to float64 autograd directly by the case c1-seeded of tests/test_gpu_production_width.py.
"""
import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

import dropout_ref as dr

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
# "distinct" has T + 1 = B = 6 steps and rows: a kernel that swapped (s, b) would transpose the seeded counter and the explicit mask alike and
# still agree with itself (seen on a deliberately wrong embed_segsum_kernel).  "rows7" differs from it in B alone, so that no two extents agree.
SHAPES = {"distinct": dict(E=72, H=64, V=301, B=6, T=5), "rows7": dict(E=72, H=64, V=301, B=7, T=5),
          "c1": dict(E=512, H=512, V=2540, B=16, T=5)}
MODELS = {"2f-f32": (2, F32), "2f-bf16": (2, BF16), "1f-f32": (1, F32), "1f-bf16": (1, BF16)}
# (shape, pdrop, seed).  One seed above 2^63: the key is a 64-bit xor, not an int.  "edge": at p = 0.5 and dr.EDGE_SEED one uniform of stream 1
# inside the small shape EQUALS p (tests/test_dropout_ref.py proves it), so `u > p` and `u >= p` give different masks there; at p = 0.4 no
# uniform can equal float32(0.4), which is no multiple of 2^-24, and the two comparisons are the same function.
DRAWS = {"distinct": ("distinct", 0.4, 0xD1CE00000000BEEF), "rows7": ("rows7", 0.4, 77), "c1": ("c1", 0.4, 123),
         "edge": ("distinct", dr.EDGE_P, dr.EDGE_SEED)}
GRID = [(s, m) for s in DRAWS for m in MODELS]


def setup(draw, model):
    shape, pdrop, seed = DRAWS[draw]
    d, (nl, dtype) = SHAPES[shape], MODELS[model]
    ctx = L.Context(d["E"], d["H"], d["H"], d["V"], max_B=d["B"], max_T=d["T"], lstm_dtype=dtype, n_layers=nl)
    ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    rng = np.random.default_rng(11)
    feats = L.to_jl((rng.standard_normal((d["B"], 4096)) * 0.05).astype(np.float32))
    tokens = rng.integers(0, d["V"], size=(d["T"], d["B"])).astype(np.int32)
    tokens[1] = tokens[0]   # repeated ids: the embedding gradient sums masked rows
    m1, m2 = dr.masks(seed, pdrop, d["T"], d["B"], d["E"], d["H"], nl)
    return ctx, feats, tokens, m1, m2, pdrop, seed


def host(ts):
    torch.cuda.synchronize()
    return [L.from_jl(t).copy() for t in ts]


def assert_same(a, b, what):
    for n, x, y in zip(L.PARAM_NAMES, a, b):
        assert x.shape == y.shape and not np.isnan(x).any()
        if not np.array_equal(x, y):
            k = np.unravel_index(np.argmax(np.abs(x - y)), x.shape)
            raise AssertionError("%s: %s differs in %d of %d elements; largest at %s: %r against %r" % (what, n, int((x != y).sum()), x.size, k, x[k], y[k]))


@pytest.mark.parametrize("draw,model", GRID, ids=["%s-%s" % g for g in GRID])
def test_seeded_run_is_bit_equal_to_the_run_with_the_transcribed_masks(draw, model):
    ctx, feats, tokens, m1, m2, pdrop, seed = setup(draw, model)
    param = L.initweights(ctx, seed=7)
    gs, ls = L.lossgradient(ctx, param, feats, tokens, pdrop=pdrop, seed=seed)
    gs = host(gs)
    gm, lm = L.lossgradient(ctx, param, feats, tokens, mask1=m1, mask2=m2)
    gm = host(gm)
    g0, l0 = L.lossgradient(ctx, param, feats, tokens)
    print("%s %s: loss seeded %.17g, masks %.17g, no dropout %.17g" % (draw, model, ls, lm, l0))
    assert ls == lm and ls != l0
    assert_same(gs, gm, "lossgradient, seed against masks")
    assert not np.array_equal(gs[6], host(g0)[6])   # the comparison is not between two runs that both ignore the mask
    fs = L.loss(ctx, param, feats, tokens, pdrop=pdrop, seed=seed)
    fm = L.loss(ctx, param, feats, tokens, mask1=m1, mask2=m2)
    assert fs == fm and fs == ls
    ctx.close()


@pytest.mark.parametrize("model", list(MODELS))
def test_one_seeded_train_step_equals_lossgradient_with_masks_plus_update(model):
    state = []
    for seeded in (True, False):
        ctx, feats, tokens, m1, m2, pdrop, seed = setup("distinct", model)   # a context each: neither run sees shadow weights the other left behind
        param = L.initweights(ctx, seed=7)
        opt = L.initparams(param)
        grads = L.zeros_like_model(param)
        if seeded:
            L.train_step(ctx, param, opt, grads, feats, tokens, pdrop=pdrop, seed=seed)
        else:
            L.lossgradient(ctx, param, feats, tokens, mask1=m1, mask2=m2, grads=grads)
            L.update(ctx, param, grads, opt)
        ctx.sync()
        assert opt.t == 1
        state.append((host(param), host(opt.m), host(opt.v)))
        ctx.close()
    for what, a, b in zip(("parameters", "first moments", "second moments"), state[0], state[1]):
        assert_same(a, b, "train_step(seed) against lossgradient(masks) + update: " + what)
    assert any(np.abs(m).max() > 0 for m in state[0][1] if m.size)
