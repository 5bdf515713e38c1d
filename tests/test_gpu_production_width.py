"""GPU: liblrcn_hip.so at the caption model's real widths, DIRECTLY against the float64 autograd transcription (tests/torch_ref.py), not
against the C oracle.  Cases by the route the row count selects, each in the `init` and the `sharp` regime (tests/production_width.py), in
f32 and bf16; each reference is computed once per process and shared between the types.  c1-seeded runs with the DEVICE-generated dropout
masks (pdrop, seed): its references take the host transcription of the counter hash (tests/dropout_ref.py) as explicit masks, so a mask
that differs from the transcription in one stream, one index or one comparison fails the same bounds; its logits are not compared.

f32: the constants of the existing f32 parity tests -- loss 1e-5 relative, gradients rtol 1e-3 + atol 1e-5, per-step logits rtol 1e-5 +
atol 1e-5 max|ref| -- and, because at init whole tensors (dW1, dWproj, dWembed: max|g| 2e-6 .. 6e-5) sit under that atol, each gradient
also per tensor in norm: ||g - g_f64|| / ||g_f64|| <= 1e-3, the same rtol with no atol beside it; they hold in both regimes (measured per tensor in norm: 2e-7 .. 2.7e-6 at init, 6e-7 .. 1.3e-5 sharp, 2.5x .. 4x the
float32 floor of 7e-8 .. 3.2e-6).  Each test prints, next to the HIP figures, the float32 floor of its case (the same transcription in torch float32 on
the CPU against float64, per tensor in norm).
bf16: against the bf16-emulating oracle -- `init`: elementwise (parity_util.assert_bf16_matches_emulation); `sharp`: per tensor in norm, at
most twice the distance between two emulating summation orders (measured: HIP 1.9e-4 .. 3.4e-3, the two orders 4e-4 .. 3.2e-3; loss HIP
2e-6 .. 8e-5, orders 8e-6 .. 1.2e-4 -- the elementwise constants' 1e-6 on the loss fails there for both) -- and independently per tensor against
float64: ||g - g_f64|| / ||g_f64|| <= max(BF16_VS_F32_GRAD_NORM, 1.5 x the emulating oracle's own distance to float64), the loss alike.
What the assertions catch, shown once on deliberately wrong builds of the library (never committed):
  the second split-K slab x 1.01 in splitk_reduce_kernel -- split-K exists for bf16 contractions only, the f32 route is gemm_nt -- fails all
  twelve bf16 cases: the per-tensor float64 bound (W1 4.03e-2 > 1.5 x 2.68e-2, Wembed 2.02e-2 > 2e-2), in sharp also the bound against
  the emulation (loss 5.3e-4 > 6.2e-5, W2 7.8e-3 > 3e-3), at init the elementwise emulation check;
  softmax_xent without the max-subtraction fails c4-rows64-sharp in both types (|logit| 121: float32 exp overflows, loss inf); every
  other case has |logit| <= 51 < 88 and cannot notice.
  The f32 norm bound is what sees a lost gradient at init: an all-zero dW1 has distance 1 and passed the elementwise check alone.
Beam search (f32): tokens identical to beam_search_ref's, probability within 1e-4; the winner's lead of 1.05 is asserted on the CPU side.
"""
import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import lrcn as L
from oracle import oracle as orc

import parity_util as pu
import production_width as pw

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
F32_GRAD_NORM = 1e-3   # ||g - g_f64|| / ||g_f64||: what rtol 1e-3 on every element amounts to over a tensor
PAIRS = [(n, r) for n in pw.GPU_CASES for r in pw.REGIMES]
ids = ["%s-%s" % p for p in PAIRS]


def run(c, dtype, logits=False, deterministic=False):
    """lossgradient (and the per-step logits) of case c on the device -> pw.Result, the route of the last contraction."""
    ctx = L.Context(c.E, c.H, c.H, c.V, max_B=c.B, max_T=c.T, lstm_dtype=dtype, n_layers=c.n_layers)
    if deterministic:
        ctx.set_option(lrcn_amd._lib.LRCN_OPT_DETERMINISTIC, 1)
    param = L.model_from_arrays(c.model.p)
    kw = dict(lens=c.lens, norm_tokens=c.norm_tokens) if c.lens is not None else dict(norm_B=c.norm_B)
    if c.pdrop is not None:   # the device's own masks, by (pdrop, seed): the references got the host transcription of them as mask1 / mask2
        kw.update(pdrop=c.pdrop, seed=c.seed)
        logits = False        # the logits entry point takes no dropout
    grads, val = L.lossgradient(ctx, param, L.to_jl(c.feats), c.tokens, **kw)
    route = L.debug_route(ctx)
    g = {n: L.from_jl(t).astype(np.float64) for n, t in zip(orc.PARAM_NAMES, grads) if n in pw.live(c.model)}
    z = L.forward_logits(ctx, param, L.to_jl(c.feats), c.tokens) if logits else None
    ctx.close()
    return pw.Result(val, g, z), route


@pytest.mark.parametrize("name,regime", PAIRS, ids=ids)
def test_f32_loss_gradients_and_logits_vs_float64_autograd(name, regime):
    c, ref = pw.case(name, regime), pw.reference(name, regime)
    pw.assert_digest(name, regime)
    got, route = run(c, F32, logits=True)
    d, dl = pw.distances(got, ref)
    fd, fdl = pw.distances(pw.reference_f32(name, regime), ref)
    print("%s %s f32: route %s; loss rel %.1e (float32 floor %.1e); per tensor HIP / floor: %s; logits max|d| / max|ref| %s" % (
        name, regime, route, dl, fdl, " ".join("%s %.1e/%.1e" % (n, d[n], fd[n]) for n in d),
        "not compared (dropout)" if got.logits is None else "%.1e" % (np.abs(got.logits - ref.logits).max() / np.abs(ref.logits).max())))
    assert dl <= 1e-5
    for n in ref.g:
        # per tensor in norm first: at init max|dW1|, max|dWproj|, max|dWembed| are below the elementwise atol of 1e-5, which alone would
        # let an all-zero gradient (distance 1) or a wrong partial sum pass.  The elementwise rtol, taken over the whole tensor, has no atol.
        assert d[n] <= F32_GRAD_NORM, (n, d[n], fd[n])
        np.testing.assert_allclose(got.g[n], ref.g[n], rtol=1e-3, atol=1e-5, err_msg=n)
    assert (got.logits is None) == (c.pdrop is not None)
    if got.logits is not None:
        np.testing.assert_allclose(got.logits, ref.logits, rtol=1e-5, atol=1e-5 * np.abs(ref.logits).max())


@pytest.mark.parametrize("name,regime", PAIRS, ids=ids)
def test_bf16_loss_and_gradients_vs_emulation_and_float64_autograd(name, regime):
    c, ref = pw.case(name, regime), pw.reference(name, regime)
    emu, emu_g = pw.oracle_result(name, regime, True)
    ed, edl = pw.distances(emu, ref)            # reference against reference: the emulation's own distance to float64
    got, route = run(c, BF16)
    d, dl = pw.distances(got, ref)
    print("%s %s bf16: route %s; loss rel %.1e (emulation %.1e); per tensor HIP / emulation vs float64: %s; HIP vs emulation: %s" % (
        name, regime, route, dl, edl, " ".join("%s %.1e/%.1e" % (n, d[n], ed[n]) for n in d),
        " ".join("%s %.1e" % (n, pw.rel_norm(got.g[n], emu.g[n])) for n in d)))
    assert dl <= max(pu.BF16_VS_F32_LOSS_RTOL, 1.5 * edl)
    for n in d:
        assert d[n] <= max(pu.BF16_VS_F32_GRAD_NORM, 1.5 * ed[n]), (n, d[n], ed[n])
    if regime == "init":
        grads = [got.g.get(n, np.zeros((0, 0))) for n in orc.PARAM_NAMES]
        pu.assert_bf16_matches_emulation(got.loss, grads, emu.loss, emu_g, "%s %s" % (name, regime))
        return
    # sharp: one flipped bf16 of h moves a logit of ~35 by ~0.1, so two EMULATING summation orders (the oracle's double- and float-
    # accumulating builds) already differ by more than the elementwise constants (parity_util's docstring).  Per tensor in norm, at most
    # twice what those two references differ by -- computed here, reference against reference, never from the HIP result.
    od, odl = pw.distances(pw.oracle_result(name, regime, True, True)[0], emu)
    hd, hdl = pw.distances(got, emu)
    print("%s sharp bf16 vs emulation, HIP / two emulating orders: loss %.1e/%.1e; %s" % (name, hdl, odl, " ".join("%s %.1e/%.1e" % (n, hd[n], od[n]) for n in hd)))
    assert hdl <= max(pu.BF16_LOSS_RTOL, 2 * odl)
    for n in hd:
        assert hd[n] <= max(pu.BF16_GRAD_NORM, 2 * od[n]), (n, hd[n], od[n])


@pytest.mark.parametrize("regime", pw.REGIMES)
def test_ordered_sums_at_1024_rows_f32_vs_float64_autograd(regime):
    """c1-rows256 on a context with LRCN_OPT_DETERMINISTIC: (T + 1) B = 1024 rows > 512, so the bias gradients come from the one-slab
    colsum_kernel<T, 64> (summed in row order) instead of the slabbed atomic form, and the embedding gradient from the sorted segmented
    sums -- forms the other deterministic tests hold only to the default route or to themselves.  Same reference, same f32 constants."""
    name = "c1-rows256"
    c, ref = pw.case(name, regime), pw.reference(name, regime)
    got, route = run(c, F32, deterministic=True)
    d, dl = pw.distances(got, ref)
    print("%s %s f32 deterministic: loss rel %.1e; per tensor %s" % (name, regime, dl, " ".join("%s %.1e" % (n, d[n]) for n in d)))
    assert dl <= 1e-5
    for n in ref.g:
        assert d[n] <= F32_GRAD_NORM, (n, d[n])
        np.testing.assert_allclose(got.g[n], ref.g[n], rtol=1e-3, atol=1e-5, err_msg=n)


@pytest.mark.parametrize("K", [3, 10])
def test_beam_search_on_the_sharp_model_vs_the_transcription(K):
    c = pw.case("c1", "sharp")
    feats, ref = pw.beam_feats(), pw.beam_reference(K)
    ctx = L.Context(c.E, c.H, c.H, c.V, max_B=pw.BEAM_IMAGES * K, max_T=4, lstm_dtype=F32)
    param = L.model_from_arrays(c.model.p)
    batch = L.beam_search_batch(ctx, param, L.to_jl(feats), K, pw.BEAM_NWORD)
    for i, (toks, prob, lead) in enumerate(ref):
        one = L.beam_search(ctx, param, L.to_jl(feats[i:i + 1]), K, pw.BEAM_NWORD)
        for what, (seq, p) in (("per image", one), ("batched", batch[i])):
            assert list(seq) == list(toks), (what, i, seq, toks)
            assert abs(p - prob) <= 1e-4 * abs(prob), (what, i, p, prob)
    ctx.close()
