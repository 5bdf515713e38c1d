"""CPU: the inputs of tests/test_gpu_xent_ladder.py meet the conditions its assertions need -- from the references alone (float64
autograd, the oracle's per-row sums, the bf16-emulating oracle in its two accumulation orders), nothing from the library under test.

1. The vocabularies sit on both sides of every rung of launch_softmax_xent, and the critical columns are what tests/xent_ladder_cases.py says.
2. |g_bout| >= 100 x the elementwise atol (1e-5) of the f32 check on every critical column of the equal-length form, so that 1 % of such
   an element stands above rtol 1e-3 + atol 1e-5.  bout's softmax mass on a critical column is only ~1e-4 .. 1e-7 at these widths, so it is
   being a target that lifts a column there: the masked forms have 6 (lens) and 5 (weighted) active token targets for up to 8 columns and
   are held to the columns they can cover -- column 0 (eos), the rung's last slot's first column and the last four columns, always.
   Measured: equal min |g_bout| 2.8e-2 .. 6.7e-2 on every critical column; lens / weighted leave 0 .. 2 / 1 .. 3 critical columns to
   their softmax mass (1e-7 .. 5e-4).
3. An inactive row (length 0, and rows that end before T) and a zero-weight row with active steps exist.
4. The +100 case overflows float32 exp without the max-subtraction, and its float64 reference is finite.
5. bf16: the elementwise rule of parity_util.assert_bf16_matches_emulation holds between the emulating oracle's two accumulation orders on
   these inputs -- measured: worst element 0.01 of its tolerance, per tensor in norm <= 5.2e-6, loss 4e-16 relative -- so the GPU test uses
   the elementwise rule, not production_width's per-tensor margin.
"""
import numpy as np
import pytest

import parity_util as pu
import xent_ladder_cases as xl
from oracle import oracle as orc


def test_vocabularies_straddle_every_rung():
    rungs = [xl.rung(V) for V in xl.VOCABS]
    assert rungs == [2, 4, 4, 8, 8, 8, 12, 12, 16, 16, 16, None]
    for last in (2048, 4096, 8192, 12288, 16384):
        assert last in xl.VOCABS and last + 1 in xl.VOCABS and xl.rung(last) != xl.rung(last + 1)
    assert [V for V in xl.VOCABS if V % 4 and xl.rung(V) == xl.rung(V - 4)] == [8190, 16383]   # a scalar tail inside a rung, not at its first column
    assert xl.critical_columns(16384) == [15360, 16383, 16382, 16381, 16380, 15359, 1024, 1023, 0]
    assert xl.critical_columns(2048) == [1024, 2047, 2046, 2045, 2044, 1023, 0]
    assert xl.critical_columns(12289) == [12288, 12287, 12286, 12285, 1024, 1023, 0]   # slots 13 .. 15 of Q = 16 hold nothing here


def test_an_inactive_row_and_a_zero_weight_row_exist():
    assert (xl.LENS == 0).any() and (xl.LENS < xl.T).any() and (xl.LENS == xl.T).any()
    zero = xl.WEIGHTS == 0
    assert zero.any() and (xl.LENS[zero] > 0).all() and (xl.WEIGHTS[~zero] > 0).all()
    assert xl.NORM_TOKENS % np.lcm.reduce(xl.LENS + 1) == 0
    assert all(q >= 1 for q in xl.wr.integer_row_norms(xl.LENS, xl.WEIGHTS, xl.NORM_TOKENS))
    assert (xl.T + 1) * xl.B == 15


@pytest.mark.parametrize("V", xl.VOCABS)
def test_targets_are_critical_columns_and_they_carry_gradient(V):
    c = xl.case(V)
    assert set(c.tokens.ravel()) <= set(c.crit) and c.tokens.min() > 0
    always = [0, c.crit[0]] + [V - k for k in (1, 2, 3, 4)]
    for form in xl.FORMS:
        r = xl.reference(V, form)
        gb = np.abs(r.g["bout"][0])
        act = [(t, b) for b in range(xl.B) for t in range(xl.T)
               if form == "equal" or (t < xl.LENS[b] and (form == "lens" or xl.WEIGHTS[b] != 0))]
        hit = {0} | {int(c.tokens[t, b]) for t, b in act}
        assert set(always) <= hit, (form, sorted(hit))
        if form == "equal":
            assert hit == set(c.crit)
        for col in hit:
            assert gb[col] >= 100 * xl.F32_ATOL, (V, form, col, gb[col])
        assert np.isfinite(r.loss) and all(np.isfinite(g).all() for g in r.g.values())


@pytest.mark.parametrize("V", xl.HOT_VOCABS)
def test_the_hot_logit_overflows_float32_exp_without_the_max_subtraction(V):
    c, r = xl.case(V, True), xl.reference(V, "equal", True)
    assert xl.rung(16384) == 16 and xl.rung(16385) is None
    assert r.logits.max() > xl.FLT_EXP_MAX and abs(r.logits[..., c.hot_col] - xl.HOT_LOGIT).max() < 1.0
    with np.errstate(over="ignore"):
        naive = np.exp(r.logits.astype(np.float32)).sum(2)
    assert np.isinf(naive).all()          # every row: softmax without the max-subtraction is inf / inf
    assert np.isfinite(r.loss) and r.loss > 50.0   # the targets are other columns: ~100 nats each
    assert np.abs(r.g["bout"][0, c.hot_col]) > 0.5


@pytest.mark.parametrize("V", xl.VOCABS)
def test_the_elementwise_bf16_rule_holds_between_the_two_emulating_orders(V):
    for form in xl.FORMS:
        e_loss, e_g = xl.emulated(V, form)
        f_loss, f_g = xl.emulated(V, form, True)
        grads = [np.asarray(f_g.p[n], np.float64) for n in orc.PARAM_NAMES]
        pu.assert_bf16_matches_emulation(f_loss, grads, e_loss, e_g, "V=%d %s, float- against double-accumulating emulation" % (V, form))
