"""GPU: the ordered bias column sums (k_colsum on a context with LRCN_OPT_DETERMINISTIC above 512 rows: colsum_kernel<T, 64>, one
1024-thread block of 64 row groups per 64 columns) against references, in both types, at the ragged shape of tests/colsum_ordered_case.py:
528 rows = 8 passes of the 64 row groups + 16 tail rows, 4 H = 288 columns (the last column block half full), V = 301 (one live column in
the last quad).  Until now the bf16 form was held only to the slabbed form and to itself, the f32 form only at 1024 rows, a multiple of 64.

f32: float64 autograd with test_gpu_production_width.py's constants -- loss 1e-5 relative, gradients rtol 1e-3 + atol 1e-5, per tensor in
norm 1e-3.
bf16: parity_util.assert_bf16_matches_emulation, the elementwise rule, against the emulating oracle.  tests/test_colsum_ordered_case.py held
the rule reference against reference first (the oracle's two accumulation orders: worst element 0.13 of its tolerance, the biases under
0.02), so production_width's per-tensor margin is not needed here.
Both: b1, b2 and bout of two calls are the same bits."""
import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import lrcn as L
from oracle import oracle as orc

import colsum_ordered_case as cc
import parity_util as pu

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
F32_GRAD_NORM = 1e-3   # test_gpu_production_width.py's


def run_twice(dtype):
    c = cc.case()
    ctx = L.Context(cc.E, cc.H, cc.H, cc.V, max_B=cc.B, max_T=cc.T, lstm_dtype=dtype)
    ctx.set_option(lrcn_amd._lib.LRCN_OPT_DETERMINISTIC, 1)
    param, fj = L.model_from_arrays(c.model.p), L.to_jl(c.feats)
    out = []
    for _ in range(2):
        grads, val = L.lossgradient(ctx, param, fj, c.tokens, norm_B=cc.B)
        out.append((val, [L.from_jl(g).astype(np.float64) for g in grads]))
    ctx.close()
    for n, a, b in zip(orc.PARAM_NAMES, out[0][1], out[1][1]):
        if n in cc.BIASES:
            assert a.tobytes() == b.tobytes(), "%s differs between two calls on a deterministic context" % n
    return out[0]


def test_ordered_sums_with_a_ragged_row_tail_f32_vs_float64_autograd():
    val, grads = run_twice(F32)
    ref = cc.reference()
    rel = abs(val - ref.loss) / abs(ref.loss)
    d = {n: cc.rel_norm(g, ref.g[n]) for n, g in zip(orc.PARAM_NAMES, grads)}
    print("f32 deterministic, 528 rows: loss %.6f (float64 %.6f, rel %.1e); per tensor %s" % (val, ref.loss, rel, " ".join("%s %.1e" % i for i in d.items())))
    assert np.isfinite(val) and rel <= 1e-5, (val, ref.loss)
    for n, g in zip(orc.PARAM_NAMES, grads):
        assert d[n] <= F32_GRAD_NORM, (n, d[n])
        np.testing.assert_allclose(g, ref.g[n], rtol=1e-3, atol=1e-5, err_msg=n)


def test_ordered_sums_with_a_ragged_row_tail_bf16_vs_emulating_oracle():
    val, grads = run_twice(BF16)
    e_loss, e_g = cc.emulated()
    print("bf16 deterministic, 528 rows: loss %.6f (emulation %.6f, rel %.1e); per tensor vs emulation %s" % (
        val, e_loss, abs(val - e_loss) / abs(e_loss), " ".join("%s %.1e" % (n, cc.rel_norm(g, e_g.p[n])) for n, g in zip(orc.PARAM_NAMES, grads))))
    pu.assert_bf16_matches_emulation(val, grads, e_loss, e_g, "colsum_kernel<bf16_t, 64>, 528 rows")
