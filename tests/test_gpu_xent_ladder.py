"""GPU: the training-side softmax + cross-entropy ladder (launch_softmax_xent, csrc/xent.hip) on both sides of every rung -- the
counterpart of tests/test_gpu_decode_wide.py's softmax_topk_rows_kernel ladder.  Cases, critical columns and references:
tests/xent_ladder_cases.py; that its inputs are decisive is asserted on the CPU (tests/test_xent_ladder_cases.py).

One context per (V, type) runs the three forms: equal lengths (softmax_xent_reg_kernel<T, Q, XENT_PLAIN>), lens (<T, Q, XENT_MASKED>) and lens + row
weights (<T, Q, XENT_WEIGHTED>); at V = 16385 the streaming softmax_xent_kernel in the same three forms.

f32: against float64 with test_gpu_production_width.py's constants -- loss 1e-5 relative, gradients rtol 1e-3 + atol 1e-5, and per tensor
||g - g_f64|| / ||g_f64|| <= 1e-3.  g_bout is the column sum of d(logits): it sees every column of every row.  At V = 16384 and 16385 a
second case has one logit of +100: without the max-subtraction float32 exp overflows and the loss is inf or nan.
bf16: parity_util.assert_bf16_matches_emulation, the ELEMENTWISE rule, against the emulating oracle with integer row norms.  The rule was
first held reference against reference on the CPU (the oracle's double- and float-accumulating orders, tests/test_xent_ladder_cases.py):
worst element 0.01 of its tolerance, per tensor in norm <= 5.2e-6, loss 4e-16 relative -- Wout at its initial scale keeps the sharpness out
of bf16 h, so production_width's per-tensor margin is not needed here.

What the assertions catch, shown once on a deliberately wrong build of the library (never committed): see test_the_ladder's docstring.
"""
import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import lrcn as L
from oracle import oracle as orc

import parity_util as pu
import xent_ladder_cases as xl

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
F32_GRAD_NORM = 1e-3   # test_gpu_production_width.py's


def run(ctx, c, **kw):
    grads, val = L.lossgradient(ctx, L.model_from_arrays(c.model.p), L.to_jl(c.feats), c.tokens, **kw)
    return val, [L.from_jl(g).astype(np.float64) for g in grads]


def assert_f32(val, grads, ref, what):
    rel = abs(val - ref.loss) / abs(ref.loss)
    d = {n: xl.rel_norm(g, ref.g[n]) for n, g in zip(orc.PARAM_NAMES, grads)}
    print("%s: loss %.6f (float64 %.6f, rel %.1e); per tensor %s" % (what, val, ref.loss, rel, " ".join("%s %.1e" % i for i in d.items())))
    assert np.isfinite(val) and rel <= 1e-5, (what, val, ref.loss)
    for n, g in zip(orc.PARAM_NAMES, grads):
        assert d[n] <= F32_GRAD_NORM, (what, n, d[n])
        np.testing.assert_allclose(g, ref.g[n], rtol=1e-3, atol=1e-5, err_msg="%s %s" % (what, n))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", xl.VOCABS)
def test_the_ladder(V, dtype):
    """A local build (not kept) whose softmax_xent_reg_kernel<., 16> added the LAST slot's exponentials x 1.01 to the row sum failed
    V = 16383 and 16384 in both types at the loss bound of the first form it met (equal; f32: rel 4.9e-5 and 4.8e-5 > 1e-5, bf16 the same
    distance > 1e-6) and the +100 case at V = 16384 (1.2e-4 > 1e-5: the hot column sits in the last slot), and passed every other case: at
    V = 12289 slot 15 of Q = 16 holds no column, and the other rungs are other instantiations."""
    c = xl.case(V)
    ctx = L.Context(xl.E, xl.H, xl.H, V, max_B=xl.B, max_T=xl.T, lstm_dtype=dtype)
    for form in xl.FORMS:
        what = "V=%d Q=%s %s %s" % (V, xl.rung(V), "f32" if dtype == F32 else "bf16", form)
        val, grads = run(ctx, c, **xl.form_kwargs(form))
        if dtype == F32:
            assert_f32(val, grads, xl.reference(V, form), what)
        else:
            e_loss, e_g = xl.emulated(V, form)
            print("%s: loss %.6f (emulation %.6f, rel %.1e); per tensor vs emulation %s" % (
                what, val, e_loss, abs(val - e_loss) / abs(e_loss),
                " ".join("%s %.1e" % (n, xl.rel_norm(g, e_g.p[n])) for n, g in zip(orc.PARAM_NAMES, grads))))
            pu.assert_bf16_matches_emulation(val, grads, e_loss, e_g, what)
    ctx.close()


@pytest.mark.parametrize("V", xl.HOT_VOCABS)
def test_a_logit_of_100_needs_the_max_subtraction_f32(V):
    c = xl.case(V, True)
    ctx = L.Context(xl.E, xl.H, xl.H, V, max_B=xl.B, max_T=xl.T, lstm_dtype=F32)
    val, grads = run(ctx, c, norm_B=xl.B)
    assert_f32(val, grads, xl.reference(V, "equal", True), "V=%d hot" % V)
    ctx.close()
