"""Shared parity checks of the GPU tests (tests/ only: imports the oracle, the checker).

bf16 kernels are compared ELEMENTWISE with the bf16-EMULATING oracle (oracle/lrcn_oracle.h, ORC_EMULATE_BF16: the same CPU
restatement of lrcn.jl rounded to bfloat16 exactly where liblrcn_hip.so stores or feeds bf16) -- what is left between the two is
summation order and the occasional one-ulp flip of a rounding whose argument differs in the last float32 bit:

    loss        |d| <= 1e-6 |loss|             (measured 3e-8 .. 5e-8; against the f32 oracle it is ~1e-7 .. 3e-7 only by luck of averaging)
    gradients   |d| <= 5e-3 |ref| + 2.5e-3 max|ref|   per element,  and  ||d|| <= 3e-3 ||ref||   per tensor
                (measured worst element 1.8e-3 max|ref| -- Wcnn, whose contraction is only B long, so one flipped bf16 of d x_cnn shows --
                 and 2e-4 .. 8e-4 for the others; the same kernels against the UN-emulated f32 oracle sit at 3e-3 .. 8e-3 max|ref|.)

A wrong 5 % term (a dropped bias column, a mis-scaled split-K slab, a stale K-padding column) moves ||d|| / ||ref|| to ~5e-2 and single
elements by 5e-2 |ref|: both bounds catch it; the cosine > 0.99 these tests used before did not.

A SECOND, INDEPENDENT bound (round 5).  The emulation's rounding points were transcribed from the HIP path, so a
rounding point that should not exist would be copied into the checker and pass.  Every caller therefore also holds the same result
against the PLAIN f32 oracle (no emulation, nothing taken from the HIP sources):

    loss        |d| <= 2e-2 |loss_f32|         (the tolerance north_star / BASELINE.md section 3 state for bf16)
    gradients   ||g - g_f32|| <= 2e-2 ||g_f32||   per tensor
                (the emulating oracle itself sits at 3e-3 .. 6e-3 of the f32 oracle at E = H = 1000: bf16 operands of 12-step recurrences;
                 an extra rounding of a whole operand class adds ~4e-3 per occurrence in quadrature, a dropped / doubled term >= 5e-2)

THE SHARP REGIME (tests/production_width.py: max |logit| 32 .. 51, 121 in c4-rows64, mean p(target) >= 0.4, saturating gates).  There the elementwise constants
fail for the emulation itself: the oracle's double- and float-accumulating builds, both emulating, differ by 8e-6 .. 1.2e-4 on the loss and
4e-4 .. 3.2e-3 per tensor in norm (one flipped bf16 of h moves a logit by ~0.1).  tests/test_gpu_production_width.py therefore holds the HIP
result (measured 2e-6 .. 8e-5 on the loss, 1.9e-4 .. 3.4e-3 per tensor) to twice the distance of those two orders, computed in the test.
"""
import numpy as np

from lrcn_amd import lrcn as L
from oracle import oracle as orc

BF16_LOSS_RTOL = 1e-6
BF16_GRAD_RTOL = 5e-3
BF16_GRAD_ATOL_FRAC = 2.5e-3
BF16_GRAD_NORM = 3e-3
BF16_VS_F32_LOSS_RTOL = 2e-2
BF16_VS_F32_GRAD_NORM = 2e-2
worst_vs_f32 = {}   # what -> (tensor, ||g - g_f32|| / ||g_f32||): the largest ratio each check saw (printed by the tests' -s runs)


def emulated_reference(model, feats, tokens, **kw):
    """loss and the nine gradients from the bf16-emulating oracle (kw: norm_B, mask1, mask2).  The gradient object also carries
    `.f32` = (loss, gradients) of the PLAIN f32 oracle on the same inputs: assert_bf16_matches_emulation applies its second bound to it."""
    with orc.emulate_bf16():
        e_loss, e_g = orc.loss(model, feats, tokens, want_grad=True, **kw)
    e_g.f32 = orc.loss(model, feats, tokens, want_grad=True, **kw)
    return e_loss, e_g


def assert_bf16_near_f32_oracle(val, grads, f32_loss, f32_g, what=""):
    """The independent bound: the bf16 result against the un-emulated f32 oracle, per tensor in norm."""
    assert abs(val - f32_loss) <= BF16_VS_F32_LOSS_RTOL * abs(f32_loss), (what, val, f32_loss)
    for n, g in zip(orc.PARAM_NAMES, grads):
        r = f32_g.p[n].astype(np.float64)
        if r.size == 0:
            continue
        a = (g if isinstance(g, np.ndarray) else L.from_jl(g)).astype(np.float64)
        rel = float(np.linalg.norm(a - r) / (np.linalg.norm(r) + 1e-300))
        if rel > worst_vs_f32.get(what, ("", 0.0))[1]:
            worst_vs_f32[what] = (n, rel)
        assert rel <= BF16_VS_F32_GRAD_NORM, "%s %s: ||g - g_f32|| / ||g_f32|| = %.3e > %g (plain f32 oracle)" % (what, n, rel, BF16_VS_F32_GRAD_NORM)


def assert_bf16_matches_emulation(val, grads, ref_loss, ref_g, what=""):
    """val / grads: what the HIP library returned (grads: device tensors in reference layout, or numpy arrays)."""
    assert abs(val - ref_loss) <= BF16_LOSS_RTOL * abs(ref_loss), (what, val, ref_loss)
    for n, g in zip(orc.PARAM_NAMES, grads):
        r = ref_g.p[n].astype(np.float64)
        if r.size == 0:
            continue
        a = (g if isinstance(g, np.ndarray) else L.from_jl(g)).astype(np.float64)
        assert a.shape == r.shape, (what, n, a.shape, r.shape)
        d = np.abs(a - r)
        mx = np.abs(r).max()
        tol = BF16_GRAD_RTOL * np.abs(r) + BF16_GRAD_ATOL_FRAC * mx
        bad = d > tol
        assert not bad.any(), "%s %s: %d of %d elements outside rtol %g + %g max|ref|; worst |d| %.3e at |ref| %.3e (max|ref| %.3e)" % (
            what, n, int(bad.sum()), r.size, BF16_GRAD_RTOL, BF16_GRAD_ATOL_FRAC, d.max(), np.abs(r).ravel()[d.argmax()], mx)
        rel = np.linalg.norm(a - r) / (np.linalg.norm(r) + 1e-300)
        assert rel <= BF16_GRAD_NORM, "%s %s: ||d|| / ||ref|| = %.3e > %g" % (what, n, rel, BF16_GRAD_NORM)
    if getattr(ref_g, "f32", None) is not None:
        assert_bf16_near_f32_oracle(val, grads, ref_g.f32[0], ref_g.f32[1], what)
