"""CPU: the C oracle (oracle/lrcn_oracle.c, hand-derived backward) held to the float64 autograd transcription (tests/torch_ref.py) at the
caption model's REAL widths -- E = H = 512 / V = 2540 and E = H = 1000 / V = 10640 -- where until now the oracle was the only reference.
Cases and the two regimes (`init`: flat softmax, linear gates; `sharp`: a trained-like model, asserted from the float64 numbers) are in
tests/production_width.py; every reference is computed once per process.  Tolerances are tests/test_oracle_golden.py's: loss 1e-6 relative,
gradients rtol 1e-4 + atol 1e-7, per-step logits rtol 1e-5 + atol 1e-6.  No GPU, no HIP library.

The oracle's loss, gradients and per-step logits come from its double-storage build (oracle/lrcn_oracle.h, orc_real): the same source,
float32 inputs widened, results returned as float32.  With float32 storage the same terms agreed to 4e-7 in norm, but in the sharp regime
0.03 % .. 0.08 % of the logits (all |ref| < 0.25 next to logits of 36 .. 51) were off by up to 3.4e-6 against atol 1e-6, and one element of
dW2 (c4-slice) by 1.16e-7 against 1.08e-7: rounding of h and of the gates, not a wrong term.  The float-storage build, which bf16
emulation and fast= still run on, is pinned to the double-storage one per tensor in norm (measured 6e-8 .. 6.2e-7 against 16 * 2^-23).

Measured (16 threads): oracle against transcription, per tensor in norm, 1e-8 .. 3.6e-8 in both regimes (the float32 rounding of the returned
gradient; torch's own float32 transcription: 1.7e-6 .. 3.3e-6); bf16-emulating oracle against float64, worst tensor: 4.7e-3 .. 6.2e-3 at
init, 1.3e-2 .. 2.7e-2 sharp.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import production_width as pw
from oracle import oracle as orc

PAIRS = [(n, r) for n in pw.CPU_CASES for r in pw.REGIMES]
ids = ["%s-%s" % p for p in PAIRS]


def test_importing_the_transcription_leaves_torch_defaults_alone():
    assert torch.get_default_dtype() == torch.float32


@pytest.mark.parametrize("name,regime", PAIRS, ids=ids)
def test_transcription_reproduces_the_committed_loss(name, regime):
    r = pw.reference(name, regime)   # asserts the sharp regime
    print("%s %s: loss %.12g  mean p(target) %.3f  |z| > 3: %.3f  max |logit| %.1f  Wout rms %s" % (
        name, regime, r.loss, r.p_target, r.saturated, r.max_logit, pw.case(name, regime).wout_rms))
    pw.assert_digest(name, regime)


@pytest.mark.parametrize("name,regime", PAIRS, ids=ids)
def test_oracle_loss_and_gradients_match_autograd(name, regime):
    ref = pw.reference(name, regime)
    got, _ = pw.oracle_result(name, regime)
    d, dl = pw.distances(got, ref)
    print("%s %s: loss rel %.1e; ||g - g_ref|| / ||g_ref||: %s" % (name, regime, dl, " ".join("%s %.1e" % kv for kv in d.items())))
    assert dl <= 1e-6
    assert set(got.g) == set(ref.g)
    for n in ref.g:
        np.testing.assert_allclose(got.g[n], ref.g[n], rtol=1e-4, atol=1e-7, err_msg=n)


FLOAT_PAIRS = [p for p in PAIRS if p[0] != "varlen"]   # mixed lengths are sums of one-row calls of the same code (tests/varlen_ref.py)
FLOAT_STORAGE_NORM = 16 * 2.0 ** -23   # 1.9e-6


@pytest.mark.parametrize("name,regime", FLOAT_PAIRS, ids=["%s-%s" % p for p in FLOAT_PAIRS])
def test_float_storage_build_stays_on_the_double_storage_one(name, regime):
    # The float-storage build is what bf16 emulation and fast= run on, and there only loose bounds look at it.  Same source, so all
    # that may separate the two builds is float32 rounding: every stored value carries up to 2^-24 relative, a step stores about a
    # dozen values in a chain (x, gates, c, h, x2, gates, c, h, logits, d logits, dz, dx) over at most 12 steps, and float exp / tanh
    # add an ulp each; independent roundings add in quadrature, sqrt(12 * 12) half-ulps = 6 * 2^-23.  16 * 2^-23 per tensor in norm leaves
    # room for that estimate and none for a wrong term (>= 1e-2).  Loss: 1e-6 relative, the golden tests' constant.
    c = pw.case(name, regime)
    val, g = orc.loss(c.model, c.feats, c.tokens, norm_B=c.norm_B, mask1=c.mask1, mask2=c.mask2, want_grad=True, wide=False)
    got = pw.Result(val, {n: np.asarray(g.p[n], np.float64) for n in pw.live(c.model)})
    d, dl = pw.distances(got, pw.oracle_result(name, regime)[0])
    print("%s %s: float storage against double storage: loss rel %.1e; %s" % (name, regime, dl, " ".join("%s %.1e" % kv for kv in d.items())))
    assert dl <= 1e-6
    for n, v in d.items():
        assert v <= FLOAT_STORAGE_NORM, (n, v)


LOGIT_PAIRS = [p for p in PAIRS if p[0] not in ("c1-masks", "c1-seeded")]   # the logits entry point takes no masks


@pytest.mark.parametrize("name,regime", LOGIT_PAIRS, ids=["%s-%s" % p for p in LOGIT_PAIRS])
def test_oracle_per_step_logits_match_the_transcription(name, regime):
    c = pw.case(name, regime)
    got = orc.forward_logits(c.model, c.feats, c.tokens)
    np.testing.assert_allclose(got, pw.reference(name, regime).logits, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name,regime", PAIRS, ids=ids)
def test_bf16_emulation_floor(name, regime):
    # the emulating oracle's own distance to float64: the floor the GPU bf16 bound of tests/test_gpu_production_width.py is sized from
    emu, _ = pw.oracle_result(name, regime, True)
    d, dl = pw.distances(emu, pw.reference(name, regime))
    print("%s %s: emulated loss rel %.1e; per tensor: %s" % (name, regime, dl, " ".join("%s %.1e" % kv for kv in d.items())))
    assert np.isfinite(dl) and dl < 3e-2
    for n, v in d.items():
        assert np.isfinite(v) and v < 3e-2, (n, v)


@pytest.mark.parametrize("K", [3, 10])
def test_beam_search_on_the_sharp_model_matches_the_transcription(K):
    c = pw.case("c1", "sharp")
    for f, (toks, prob, lead) in zip(pw.beam_feats(), pw.beam_reference(K)):
        assert lead >= pw.BEAM_MARGIN, lead   # the winner leads in float64: token equality is a fair demand of float32 products
        seq, p = orc.beam_search(c.model, f, K, pw.BEAM_NWORD)
        assert list(seq) == list(toks), (seq, toks)
        assert abs(p - prob) <= 1e-5 * abs(prob)


@pytest.mark.parametrize("Cin,Cout,W,H", [(3, 64, 14, 14), (64, 64, 14, 14), (128, 256, 14, 14), (512, 512, 14, 14), (64, 64, 10, 14)])
def test_conv_oracle_at_real_channel_counts(Cin, Cout, W, H):
    # every GPU convolution test trusts orc.conv3x3; independently pinned so far only at Cin = 5, Cout = 7 (cnn_small.npz).
    # Julia (W,H,C,N) column-major == torch [N][C][H][W]: reverse the axes.
    rng = np.random.default_rng(Cin + Cout + W)
    N = 2
    x = rng.standard_normal((N, Cin, H, W)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    jl = lambda a: np.transpose(a, (3, 2, 1, 0))
    lin = F.conv2d(t(x), t(w), t(b), padding=1)

    def close(got, ref):
        ref = ref.numpy()
        np.testing.assert_allclose(got, jl(ref), rtol=1e-5, atol=1e-6 * np.abs(ref).max())

    close(orc.conv3x3(jl(x), jl(w), b, relu=False), lin)
    y = orc.conv3x3(jl(x), jl(w), b, relu=True)
    close(y, F.relu(lin))
    close(orc.pool2(y), F.max_pool2d(F.relu(lin), 2))
    yp = F.max_pool2d(F.relu(lin), 2)
    K, O = Cout * (H // 2) * (W // 2), 11
    w6 = (rng.standard_normal((O, K)) * 0.05).astype(np.float32)
    b6 = rng.standard_normal(O).astype(np.float32)
    f = t(w6) @ yp.reshape(N, K).T + t(b6)[:, None]
    got = orc.fc(w6, b6, orc.pool2(y).reshape(-1, N, order="F"), relu=False)
    np.testing.assert_allclose(got, f.numpy(), rtol=1e-5, atol=1e-6 * float(f.abs().max()))
