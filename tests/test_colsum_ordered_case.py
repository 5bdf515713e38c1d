"""CPU: the shape of tests/test_gpu_colsum_ordered.py is the ragged one its docstring says, its float64 reference gives the critical bias
columns a gradient the f32 bounds can see, and -- reference against reference, nothing from the library -- the elementwise bf16 rule of
parity_util.assert_bf16_matches_emulation holds between the emulating oracle's double- and float-accumulating orders at this shape, with
the margin printed.  (Measured: worst element 0.13 of its tolerance -- Wcnn, the biases 0.013, 0.004 and 0.0002 -- per tensor in norm
<= 2.2e-4 of the allowed 3e-3, loss 2.3e-8 relative of the allowed 1e-6 -- so the GPU test uses the elementwise rule, as tests/test_gpu_xent_ladder.py does, not production_width's per-tensor
margin.)"""
import numpy as np

import colsum_ordered_case as cc
import parity_util as pu
from oracle import oracle as orc


def test_the_shape_is_ragged_in_rows_column_blocks_and_quads():
    assert cc.ROWS == 528 and cc.ROWS > 512                     # above k_colsum's one-slab row count: the 64-row-group form when deterministic
    assert cc.ROWS // 64 == 8 and cc.ROWS % 64 == 16            # 8 full passes + 16 tail rows
    assert (4 * cc.H) // 64 == 4 and (4 * cc.H) % 64 == 32      # the last block of b1 / b2 is half full
    assert cc.V % 4 == 1 and cc.V % 64 == 45                    # one live column in bout's last quad
    c = cc.case()
    assert c.tokens.shape == (cc.T, cc.B) and 0 <= c.tokens.min() and c.tokens.max() == cc.V - 1
    assert (c.tokens[:, 32:] == cc.V - 1).any()                 # ... and it is a target in rows 32 .. 47 of a step: the tail rows of step T
    #                                                             are rows 32 .. 47 of the last step, whose target is eos for every row


def test_bias_gradients_are_visible_to_the_f32_bounds():
    """The f32 check is rtol 1e-3 + atol 1e-5 per element and 1e-3 per tensor in norm.  A sum that lost its 16 tail rows, or its last
    column block, moves a bias gradient by a few percent of its norm; for the elementwise part to see single columns too, the critical
    columns (the last live one of bout, the first of its last block, the last of b1 / b2) stand at least 100 x atol high."""
    g = cc.reference().g
    assert abs(g["bout"][0, cc.V - 1]) >= 1e-3 and abs(g["bout"][0, 256]) >= 1e-3, (g["bout"][0, cc.V - 1], g["bout"][0, 256])
    for n in ("b1", "b2"):
        a = np.abs(g[n]).ravel()
        assert a.shape == (4 * cc.H,) and a[256:].max() >= 1e-3, (n, a[256:].max())
        # (the median |g| of b1 is 7e-5, a few atol: most single columns of b1 / b2 are held by the per-tensor norm, which has no atol)
    # step T's rows alone (targets eos): bout's eos column collects them -- the largest single share of the tail
    assert abs(g["bout"][0, 0]) >= 1e-2


def test_the_elementwise_bf16_rule_holds_between_the_two_emulating_orders():
    e_loss, e_g = cc.emulated()
    f_loss, f_g = cc.emulated(True)
    worst = 0.0
    for n in orc.PARAM_NAMES:
        r, a = np.asarray(e_g.p[n], np.float64), np.asarray(f_g.p[n], np.float64)
        tol = pu.BF16_GRAD_RTOL * np.abs(r) + pu.BF16_GRAD_ATOL_FRAC * np.abs(r).max()
        worst = max(worst, float((np.abs(a - r) / tol).max()))
        print("%-6s worst element %.3g of its tolerance; in norm %.3g of %g" % (n, (np.abs(a - r) / tol).max(), cc.rel_norm(a, r), pu.BF16_GRAD_NORM))
    print("loss: %.3g relative of %g allowed; worst element over all tensors %.3g of its tolerance" % (
        abs(f_loss - e_loss) / abs(e_loss), pu.BF16_LOSS_RTOL, worst))
    grads = [np.asarray(f_g.p[n], np.float64) for n in orc.PARAM_NAMES]
    pu.assert_bf16_matches_emulation(f_loss, grads, e_loss, e_g, "colsum shape, float- against double-accumulating emulation")
    assert worst <= 0.5 and abs(f_loss - e_loss) <= 0.5 * pu.BF16_LOSS_RTOL * abs(e_loss)   # with margin: at most half the rule
