"""CPU: the width table of tests/width_cases.py keeps the properties it is there for, the references the GPU file leans on hold at these
widths, and every decode case is free of tied hypotheses.  No GPU.

1. Table properties: every residue of H1 modulo 4, every valid-unit count 1..7 of the 8-unit recurrence forms among the widths those forms
   accept (H >= 16), a width of 17 K-tiles, a width under 16, H1 != H2, an E off the vector grid with H on it.  The activity sets (five, as
   the issue lists them) carry the off-grid residues 1, 2 and 3, the 17 K-tiles, the width under 16 and, among their eligible widths, the
   unit counts 1 and 2; the other counts run in the caption sets (both models launch the same recurrence kernels).
2. For every caption set at a tiny batch: the f32 oracle (oracle/) against the float64 autograd transcription (tests/torch_ref.py) by the
   bounds of tests/test_oracle_production_width.py (loss 1e-6 relative, gradients rtol 1e-4 + atol 1e-7), and the bf16-emulating oracle
   against the f32 oracle by parity_util.assert_bf16_near_f32_oracle.  The activity references (tests/activity_ref.py): emulated(bf16=False),
   the hand-written backward, against reference(), the autograd one.
   For the Adam trajectory sets: width_cases.adam_reference's ill-conditioned elements are few, and outside them the oracle's own
   float-storage build follows its double-storage build within the 5e-6 the GPU file asserts there.
3. Every decode case's float64 beam (tests/torch_ref.py) has a winner that leads by width_cases.TIE_MARGIN, as
   tests/test_gpu_context_reuse.py::test_decode_inputs_have_no_tied_hypotheses asserts for its own inputs.
"""
import numpy as np
import pytest
import torch

import activity_ref
import torch_ref as tr
import width_cases as wc
from oracle import oracle as orc
from parity_util import assert_bf16_near_f32_oracle

B_TINY, T_TINY = 3, 3


# ---------------------------------------------------------------------------------------------- 1. the table
def test_caption_table_properties():
    two = [wc.CAPTION[n] for n in wc.TWO_LAYER]
    assert {d[1] % 4 for d in two} == {0, 1, 2, 3}
    hs = [h for d in wc.CAPTION.values() for h in d[1:3]]
    fused = [h for h in hs if h >= wc.FUSED_MIN_H]   # lstm_fused_eligible: narrower layers never reach the step kernels
    assert {wc.last_units(h, 8) for h in fused} >= set(range(1, 8)), sorted({wc.last_units(h, 8) for h in fused})
    assert {5, 7, 9} <= {wc.last_units(d[1], 12) for d in two if d[1] >= wc.FUSED_MIN_H}   # the 12-unit forms beside the convolutions
    assert any(d[0] % 4 and not (d[1] | d[2]) & 3 and min(d[1:3]) > 64 for d in two)   # E off the grid where every route predicate accepts
    assert any(wc.ld64(h) // 64 == 17 for h in hs) and any(h < 16 for h in hs)
    assert any(d[0] > 1024 for d in two) and any(d[0] % 4 == 1 for d in two)   # E: above 1024; the embed_segsum tail
    assert any(d[1] != d[2] and not (d[1] | d[2]) & 3 for d in two)        # H1 != H2 on the vector grid: that factor alone
    assert all(d[2] % 2 == 0 and d[2] >= 2 and d[3] >= 3 for d in wc.CAPTION.values())   # what lrcn_create accepts
    assert all(d[1] == d[2] for n, d in wc.CAPTION.items() if d[4] == 1)
    assert wc.CAPTION["min"][:4] == (1, 1, 2, 3)
    assert {(wc.CAPTION[n][1] > 64, wc.CAPTION[n][1] % 4 == 0) for n in ("mid_odd", "edge64", "edge68")} == {(True, False), (False, True), (True, True)}
    assert {v % 4 for _, v in wc.DECODE_ROUTES.values()} == {0, 1, 2} and all(v >= 256 for _, v in wc.DECODE_ROUTES.values())
    e, h1, h2 = wc.CAPTION["over1024"][:3]
    assert wc.ld64(h1) // 64 == wc.ld64(h2) // 64 == 17 and wc.ld64(4 * h1) > 4 * h1 and wc.ld64(4 * h2) > 4 * h2 and e % 4 == 1


def test_activity_table_properties():
    hs = [h for _, h, _ in wc.ACTIVITY]
    assert {h % 4 for h in hs} >= {1, 2, 3}
    assert any(wc.ld64(h) // 64 == 17 for h in hs) and any(h < 16 for h in hs) and min(hs) == 1
    assert {wc.last_units(h, 8) for h in hs if h >= wc.FUSED_MIN_H} == {1, 2}   # 50, 17 and 1041; 15 (7 units) and 1 stay on GEMM + cell
    assert any(f % 4 for f, _, _ in wc.ACTIVITY)


# ---------------------------------------------------------------------------------------------- 2. the references at these widths
def _torch_params(m, requires_grad=False):
    return {n: torch.tensor(m.p[n], dtype=torch.float64, requires_grad=requires_grad) for n in orc.PARAM_NAMES if m.p[n].size}


def _t(a):
    return None if a is None else torch.tensor(a, dtype=torch.float64)


@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masks"])
@pytest.mark.parametrize("name", list(wc.CAPTION))
def test_oracle_matches_float64_autograd_and_emulation_stays_near(name, masks):
    m, c = wc.model(name), wc.batch(name, B_TINY, T_TINY, masks)
    p = _torch_params(m, True)
    if m.n_layers == 1:
        val = tr.loss1(p, _t(c.feats), c.tokens, c.B, _t(c.mask1))
    else:
        val = tr.loss(p, _t(c.feats), c.tokens, c.B, _t(c.mask1), _t(c.mask2))
    val.backward()
    ref = float(val.detach())
    got, g = orc.loss(m, c.feats, c.tokens, mask1=c.mask1, mask2=c.mask2, want_grad=True)
    assert abs(got - ref) <= 1e-6 * abs(ref), (got, ref)
    for n in p:
        np.testing.assert_allclose(g.p[n], p[n].grad.numpy(), rtol=1e-4, atol=1e-7, err_msg=n)
    # the emulation at the smallest batch the GPU file runs (at B = 3 the 1 x 1 dWproj of `min` is a sum of 12 bf16-rounded terms and the
    # emulation itself sits 9.3e-2 from the f32 oracle; from 21 rows every set stays under 8e-3, measured)
    c = wc.batch(name, wc.B_SMALL, T_TINY, masks)
    got, g = orc.loss(m, c.feats, c.tokens, mask1=c.mask1, mask2=c.mask2, want_grad=True)
    with orc.emulate_bf16():
        e_loss, e_g = orc.loss(m, c.feats, c.tokens, mask1=c.mask1, mask2=c.mask2, want_grad=True)
    assert_bf16_near_f32_oracle(e_loss, [e_g.p[n] for n in orc.PARAM_NAMES], got, g, "emulation %s" % name)


@pytest.mark.parametrize("shape", wc.ACTIVITY, ids=["F%d-H%d-C%d" % s for s in wc.ACTIVITY])
def test_activity_references_agree(shape):
    F, H, C_ = shape
    T, B = 4, 3
    rng = np.random.default_rng(H)
    P = [rng.standard_normal(s) * 0.3 for s in ((F + H, 4 * H), (1, 4 * H), (H, C_), (1, C_))]
    x, lab, lens = wc.activity_inputs(F, H, C_, T, B)
    rl, rg, rc, rf = activity_ref.reference(*P, x, lab, lens, T, B)
    el, eg, ec, ef = activity_ref.emulated(*P, x, lab, lens, T, B, bf16=False)
    assert abs(el - rl) <= 1e-12 * abs(rl)
    for a, b in zip(eg, rg):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(b).max()))
    np.testing.assert_allclose(ec, rc, rtol=1e-12)
    np.testing.assert_allclose(ef, rf, rtol=1e-12)


@pytest.mark.parametrize("name", wc.ADAM_SETS)
def test_adam_trajectory_is_well_conditioned_outside_the_recorded_elements(name):
    """width_cases.adam_reference: the count of ill-conditioned elements stays at what width_cases.ADAM_ILL records (measured: 143 of 141074,
    19 of 59263, 99380 of 20.2 M, 72 of 136528; at most 1 % of a tensor), and on all other elements three steps of orc.adam on the
    float-storage build's gradients end within ADAM_ATOL of the same steps on the double-storage build's: the reference itself holds the
    bound there.  Every element of the same pair stays within adam_reference's .bound."""
    r = wc.adam_reference(name)
    count, total = wc.ADAM_ILL[name]
    assert sum(a.size for a in r.ill.values()) == total
    got = sum(int(a.sum()) for a in r.ill.values())
    print("%s: %d of %d elements ill-conditioned" % (name, got, total))
    assert abs(got - count) <= 0.1 * count, (got, count)
    assert all(a.mean() <= 1e-2 for a in r.ill.values()), {n: float(a.mean()) for n, a in r.ill.items()}
    for n in r.params:
        d = np.abs(r.float_params[n].astype(np.float64) - r.params[n])
        assert (d[~r.ill[n]] <= wc.ADAM_ATOL).all(), (n, float(d[~r.ill[n]].max()))
        assert (d <= r.bound[n]).all(), n


# ---------------------------------------------------------------------------------------------- 3. decodes without ties
@pytest.mark.parametrize("key", list(wc.DECODES))
def test_decode_inputs_have_no_tied_hypotheses(key):
    d = wc.DECODES[key]
    m = wc.decode_model(d.name, d.V)
    p = _torch_params(m)
    beam = tr.beam_search_ref1 if m.n_layers == 1 else tr.beam_search_ref
    worst, lens = np.inf, set()
    for f in wc.decode_feats(d.N):
        xs = beam(p, torch.tensor(f[None], dtype=torch.float64), d.K, wc.NWORD)
        worst = min(worst, float(xs[0][1]) / float(xs[1][1]))
        lens.add(len(xs[0][0]))
        # and the C oracle, which the GPU file compares with, decodes what the transcription decodes
        seq, prob = orc.beam_search(m, f, d.K, wc.NWORD)
        assert list(seq) == list(xs[0][0]), (key, list(seq), xs[0][0])
        assert abs(prob - float(xs[0][1])) <= 1e-5 * float(xs[0][1])
    print("%s: smallest winner / runner-up ratio %.9f, caption lengths %s" % (key, worst, sorted(lens)))
    assert worst >= wc.TIE_MARGIN, worst
    assert key == "min" or max(lens) > 2   # captions, not just [bos, eos]
