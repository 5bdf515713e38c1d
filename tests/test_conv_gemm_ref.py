"""CPU: the references and the case table of the GEMM engines' convolution-mode tests (tests/conv_gemm_ref.py) are right before any kernel
is judged by them.

Every case of the table is built here, which asserts its input conditions (integer regime: 9 Cin max|x| max|w| + max|bias| < 2^24, both
signs before the ReLU, at least half of the written values above 2^8 and some above 2^11).  Both references are then held against an
independent computation, torch.nn.functional.conv2d on the same operands: in the integer regime the f32 conv2d must equal the float64
reference exactly (the very claim the GPU test rests on: any f32 summation order is exact), in the real-valued regime the float64 conv2d
must agree to float64 rounding and the f32 conv2d -- some f32 summation order -- must lie inside the derived bound.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_gemm_ref as cr
import gemm_ref as gr


def test_table_covers_every_rung_twice_in_both_output_modes():
    ids = [c.id for c in cr.CASES]
    assert len(ids) == len(set(ids)), "two cases share an id"
    assert 100 <= len(ids) <= 130, len(ids)
    for rung in cr.RUNGS:
        for pool in (False, True):
            hit = [c for c in cr.CASES if c.pool == pool and (c.route == rung or c.route.startswith(rung + ":"))]
            shapes = {c.operands_key for c in hit if not c.wg_cap}
            if rung == "8p:2":   # one shape (400 row tiles of 512: 204544 rows) plus its capped run
                assert len(shapes) >= 1 and any(c.wg_cap for c in hit), (rung, pool)
            else:
                assert len(shapes) >= 2, (rung, pool, len(shapes))
    assert all(c.route.split(":")[0] in {r.split(":")[0] for r in cr.RUNGS} for c in cr.CASES)
    # the persistent walk: both 8p tile shapes, the 512-row tile and the split-K form under a cap
    assert {c.route for c in cr.CASES if c.wg_cap} >= {"8p:0", "8p:1", "8p:2", "8p-splitk:6"}
    # an implicit-GEMM engine decodes pixels from (H, W): every rung sees W != H
    for rung in cr.RUNGS:
        if rung != "8p:2":
            assert any(c.W != c.H for c in cr.CASES if c.route.split(":")[0] == rung.split(":")[0]), rung


def test_real_valued_regime_covers_the_listed_routes_in_both_output_modes():
    real = [c for c in cr.CASES if c.regime == "real"]
    assert len({c.operands_key for c in real}) >= 6
    for route in cr.REAL_ROUTES:
        for pool in (False, True):
            assert any(c.pool == pool and (c.route == route or c.route.startswith(route + ":")) for c in real), (route, pool)


def test_layout_has_margins_guards_and_lead_ins():
    cs = next(c for c in cr.CASES if c.pad_c and c.pool)
    p = cr.Problem(cs)
    ce = gr.chunk(cs.dtype)
    assert p.xm >= (cs.W + 1) * cs.Cin + 64 and p.xm % ce == 0
    assert (p.x_flat[:p.xm] == gr.OPERAND_PAD).all() and (p.x_flat[-p.xm:] == gr.OPERAND_PAD).all()
    assert p.x.shape == (cs.N, cs.H, cs.W, cs.Cin) and not (p.x == gr.OPERAND_PAD).any()
    assert (p.w_flat[:p.off_w] == gr.OPERAND_PAD).all() and (p.w[cs.Cout] == gr.OPERAND_PAD).all() and p.off_w > 0
    assert cs.ldc == cs.Cout + 8 and p.y.shape == (cs.M // 4 + 1, cs.ldc)
    assert (p.y[:, cs.Cout:] == gr.C_SENTINEL).all() and (p.y[cs.out_rows] == gr.C_SENTINEL).all() and (p.y_flat[:p.off_c] == gr.C_SENTINEL).all()
    assert (p.y[:cs.out_rows, :cs.Cout] == gr.C_STALE).all()
    for c in cr.CASES:   # 16-byte aligned, not page aligned, whatever the geometry
        for off_bytes in (cr.x_margin(c) * 16 // gr.chunk(c.dtype), cr.LEAD * 16):
            assert off_bytes % 16 == 0 and off_bytes % 4096 != 0, (c.id, off_bytes)


def _conv2d(p, dtype):
    """torch's own convolution of the case's operands in `dtype`, + bias, ReLU, 2x2 maximum: [out_rows][Cout]."""
    cs = p.case
    x = p.x.to(dtype).permute(0, 3, 1, 2)                                          # NCHW
    w = p.w[:cs.Cout].to(dtype).view(cs.Cout, 3, 3, cs.Cin).permute(0, 3, 1, 2)    # [Cout][Cin][kh][kw]
    y = F.conv2d(x, w, bias=p.bias.to(dtype) if cs.bias else None, padding=1)
    if cs.relu:
        y = F.relu(y)
    if cs.pool:
        y = F.max_pool2d(y, 2)
    return y.permute(0, 2, 3, 1).reshape(cs.out_rows, cs.Cout)


@pytest.mark.parametrize("cs", cr.CASES, ids=[c.id for c in cr.CASES])
def test_case_conditions_and_reference_vs_torch_conv2d(cs):
    p = cr.Problem(cs)   # asserts the input conditions of an integer-regime case
    t32 = _conv2d(p, torch.float32)
    if cs.regime == "int":
        assert np.array_equal(t32.double().numpy(), p.ref)
        want = t32 if cs.dtype == gr.F32 else t32.bfloat16()
        assert want.dtype == p.expected.dtype and np.array_equal(gr.bits(want), gr.bits(p.expected))
        if cs.dtype == gr.BF16:   # the bf16 rounding is a real one for these magnitudes: the table can tell a truncation from a rounding
            assert (p.expected.float() != t32).any()
    else:
        t64 = _conv2d(p, torch.float64).numpy()
        assert np.abs(t64 - p.ref).max() <= 1e-12 * np.abs(p.ref).max()
        got = t32.double().numpy() if cs.dtype == gr.F32 else t32.bfloat16().double().numpy()
        assert (np.abs(got - p.ref) <= p.bound).all()


def test_tap_order_is_kh_major():
    """w[co][kh * 3 + kw][c] multiplies x[n][y + kh - 1][x + kw - 1][c]: one weight at tap (0, 2) moves the image down-left by (1, -1)."""
    x = torch.arange(2 * 4 * 6 * 1, dtype=torch.float64).view(2, 4, 6, 1) + 1
    w = torch.zeros(1, 9, 1, dtype=torch.float64)
    w[0, 0 * 3 + 2, 0] = 1.0
    y = cr.conv_taps(x, w)[..., 0]
    assert torch.equal(y[:, 1:, :-1], x[:, :-1, 1:, 0]) and (y[:, 0] == 0).all() and (y[:, :, -1] == 0).all()
    assert torch.equal(cr.pool2(x)[0, 1, 2, 0], x[0, 2:4, 4:6, 0].max())


def test_expected_bits_tell_a_nearly_right_engine_from_an_exact_one():
    """Host restatements of the slips the loose bounds let through, on one small case: each changes the expected bits."""
    cs = next(c for c in cr.CASES if c.route == "8p-splitk:2" and c.W != c.H and not c.relu and not c.pool)
    p = cr.Problem(cs)
    x64, w64 = p.x.double(), p.w[:cs.Cout].double()
    e = p.expected.float().view(cs.N, cs.H, cs.W, cs.Cout)

    def finish(conv):
        return conv.float().bfloat16().float()   # no bias, no ReLU in this case: one rounding

    # (1) tap (2, 2) not masked on the right border column: the engine's address is the pixel W + 1 further on in the flat allocation --
    # the next row's first pixel, or behind the last image x's margin of 2^15
    flat = p.x_flat.double()
    idx = (torch.arange(cs.N * cs.H) * cs.W + cs.W - 1 + cs.W + 1) * cs.Cin + p.xm
    stray = torch.stack([flat[i:i + cs.Cin] for i in idx.tolist()]) @ w64[:, 8, :].T            # [N * H][Cout]
    col = (cr.conv_taps(x64, w64)[:, :, cs.W - 1] + stray.view(cs.N, cs.H, cs.Cout))
    wrong = finish(col)
    assert (wrong != e[:, :, cs.W - 1]).any(dim=2).all()                   # every pixel of that column differs
    assert (wrong[-1, -1] - e[-1, -1, cs.W - 1]).abs().max() > 2.0 ** 15   # ... and the one that read the margin loudly
    # (2) the K-tile at the split-K seam (tap 4 of channel slice 1) counted twice
    twice = x64[..., 64:128].reshape(-1, 64) @ w64[:, 4, 64:128].T
    wrong = finish(cr.conv_taps(x64, w64) + twice.view(cs.N, cs.H, cs.W, cs.Cout))
    assert (wrong != e).float().mean() > 0.9
    # (3) a pool window taken over rows (1, 2) instead of (0, 1) in one tile corner
    full = finish(cr.conv_taps(x64, w64))
    right, shifted = cr.pool2(full[:1, 0:2, 0:2]), cr.pool2(full[:1, 1:3, 0:2])
    assert (right != shifted).any()
    # (4) a truncating conversion to bf16 instead of round-to-nearest-even
    f32 = cr.conv_taps(x64, w64).float()
    trunc = (f32.view(torch.int32) & -65536).view(torch.float32)
    assert (trunc != e).float().mean() > 0.2


def test_integer_conditions_reject_small_magnitudes(monkeypatch):
    monkeypatch.setattr(cr, "_int_magnitude", lambda K: 1)   # results of a few units: exact in bf16, would prove nothing
    cr._operands.cache_clear()
    try:
        with pytest.raises(AssertionError):
            cr.Problem(cr.Case("gemm_nt", 6, 10, 2, 64, 72))
    finally:
        cr._operands.cache_clear()


def test_where_names_image_row_and_column():
    cs = cr.Case("gemm_nt", 6, 10, 2, 64, 72, pool=True)
    n, y, x = cr.where(cs, [0, 14, 15, 29])
    assert list(n) == [0, 0, 1, 1] and list(y) == [0, 4, 0, 4] and list(x) == [0, 2, 0, 2]
