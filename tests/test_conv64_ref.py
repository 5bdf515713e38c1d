"""CPU: the references and case tables of tests/conv64_ref.py hold what tests/test_gpu_conv64_exact.py relies on.

Every case builds and meets its input conditions (they are asserted where the operands are made); the fused reference equals the oracle's
bf16-emulating chain bit for bit on its two smallest cases -- a second, independent restatement, in the reference's layouts; and the grid
and walk lengths each table row claims are recomputed from the launchers' rule (launch_conv64 / launch_conv64_fused11 / launch_conv64f:
(cap >= 8 ? cap : 256) / chunks workgroups, at least one, at most one per tile; workgroup b walks tiles b, b + G, ...).
"""
import numpy as np
import pytest
import torch

import conv64_ref as c6
import gemm_ref as gr
from oracle import oracle as orc


@pytest.mark.parametrize("cs", c6.PLAIN_CASES, ids=[c.id for c in c6.PLAIN_CASES])
def test_plain_case_builds_and_meets_its_conditions(cs):
    p = c6.Problem(cs)   # check_int_conditions runs inside
    assert cs.Cin == 64 and cs.route == "conv64" and cs.dtype == gr.BF16 and cs.regime == "int" and cs.ldc == cs.Cout
    assert p.expected.dtype == torch.bfloat16 and tuple(p.expected.shape) == (cs.out_rows, cs.Cout)
    assert cs.W % 16 == 0 and cs.H % 16 == 0 and cs.Cout % 64 == 0
    assert p.xm >= (cs.W + 1) * 64 + 64 and float(p.x_flat[0]) == gr.OPERAND_PAD == float(p.x_flat[-1])
    assert (p.bias is not None) == cs.relu


def test_plain_table_is_the_issue_table():
    rows = {}
    for cs in c6.PLAIN_CASES:
        rows.setdefault((cs.W, cs.H, cs.N, cs.Cout, cs.wg_cap), []).append((cs.relu, cs.pool))
    assert set(rows) == set(c6.PLAIN_WALKS)
    with_relu = {(48, 32, 3, 64, 8), (32, 32, 5, 128, 8), (48, 48, 3, 128, 8), (16, 16, 87, 192, 0)}
    for key, variants in rows.items():
        want = [(r, p) for r in ((False, True) if key in with_relu else (False,)) for p in (False, True)]
        assert variants == want, key
    assert len({cs.id for cs in c6.PLAIN_CASES}) == len(c6.PLAIN_CASES) == 22


@pytest.mark.parametrize("key", sorted(c6.PLAIN_WALKS), ids=["%dx%dx%d-%d-cap%d" % k for k in sorted(c6.PLAIN_WALKS)])
def test_plain_grid_and_walks(key):
    W, H, N, Cout, cap = key
    tiles, G, lengths = c6.PLAIN_WALKS[key]
    assert tiles == N * (H // 16) * (W // 16)
    assert c6.grid(tiles, Cout // 64, cap) == G
    w = c6.walks(tiles, G)
    assert sum(w) == tiles and set(w) == lengths, (key, w)


def test_plain_walks_reach_what_the_table_says():
    w = {k: c6.walks(v[0], v[1]) for k, v in c6.PLAIN_WALKS.items()}
    assert w[(16, 16, 1, 64, 0)] == [1]                                   # tile_at(1) = -1 in the prologue
    assert w[(48, 32, 3, 64, 8)] == [3, 3, 2, 2, 2, 2, 2, 2]
    assert w[(32, 32, 5, 128, 8)] == [5, 5, 5, 5]                         # j = 3, 4: the three-patch ring wraps
    assert w[(48, 48, 3, 128, 8)] == [7, 7, 7, 6]
    assert 8 // (576 // 64) == 0 and w[(16, 32, 2, 576, 8)] == [4]        # cap / chunks = 0 -> 1
    assert 256 // 3 == 85 and sorted(w[(16, 16, 87, 192, 0)]) == [1] * 83 + [2, 2]
    assert sorted(w[(16, 16, 258, 64, 0)]) == [1] * 254 + [2, 2]
    # 48 x 48 is 3 x 3 tiles per image: tile 4 of each image (ty = tx = 1) touches no border, and workgroup 0 walks image 0's (tile 4)
    assert 4 in range(0, 27, 4) and (4 % 9) // 3 == 1 and (4 % 9) % 3 == 1


@pytest.mark.parametrize("key", c6.FUSED_CASES, ids=["S%d-N%d-cap%d" % k for k in c6.FUSED_CASES])
def test_fused_case_builds_meets_its_conditions_and_walks(key):
    S, N, cap = key
    f = c6.fused(S, N)   # Stage1.check and Fused.check run inside
    print("S=%d N=%d: head2 %.3g, one-signed sum %.0f, cuts %.2f / %.2f, a1 rounded %.2f, outputs above 2^8 %.2f" % (
        S, N, f.head2, f.side, float((f.s1.pre1 < 0).double().mean()), f.cut2, f.s1.moved, f.big))
    assert tuple(f.expected.shape) == (N, S // 2, S // 2, 64) and f.expected.dtype == torch.bfloat16
    tiles, G, lengths = c6.FUSED_WALKS[key]
    assert tiles == N * (S // 16) ** 2 and c6.grid(tiles, 1, cap) == G
    w = c6.walks(tiles, G)
    assert sum(w) == tiles and set(w) == lengths, (key, w)


def test_fused_tables_agree():
    assert set(c6.FUSED_WALKS) == set(c6.FUSED_CASES) and len(c6.FUSED_CASES) == 8
    assert c6.CONV11_CASES == [(6, 1), (16, 1), (18, 3), (224, 1)]


@pytest.mark.parametrize("S,N", c6.CONV11_CASES)
def test_conv11_case_builds_and_meets_its_conditions(S, N):
    s = c6.stage1(S, N)
    assert tuple(s.a1.shape) == (N, S, S, 64) and (s.a1 == 0).any() and (s.a1 > 256).any()
    # the float source holds the same integers as the uint8 source minus the integer means
    assert torch.equal(s.x, s.x.round()) and float(s.x.min()) >= -124 and float(s.x.max()) <= 151


@pytest.mark.parametrize("S,N", [(16, 1), (32, 3)])
def test_fused_reference_equals_the_emulating_oracle(S, N):
    """orc.preprocess_u8, then orc.conv3x3 twice and orc.pool2 under orc.emulate_bf16(), on the same operands in the reference's layouts."""
    f = c6.fused(S, N)
    s = f.s1
    mean = np.array(c6.MEAN, np.float32)
    x = orc.preprocess_u8(s.img.numpy(), mean)
    assert np.array_equal(x, c6.to_ref_x(s.x).float().numpy())
    w11 = np.asfortranarray(c6.to_ref_w(s.w11).float().numpy())
    w12 = np.asfortranarray(c6.to_ref_w(f.w12).float().numpy())
    with orc.emulate_bf16():
        a1 = orc.conv3x3(x, w11, s.b11.float().numpy(), relu=True)
        out = orc.pool2(orc.conv3x3(a1, w12, f.b12.float().numpy(), relu=True))
    assert torch.equal(c6.from_ref_y(a1), s.a1.float())
    assert torch.equal(c6.from_ref_y(out), f.expected.float())


def test_three_piece_bias_values():
    hi, mid, lo = c6.bf16_pieces(torch.tensor([300.00390625, 513.51171875, -64.5]))
    assert (hi + mid + lo).tolist() == [300.00390625, 513.51171875, -64.5]
    assert float(lo[0]) == 0.0 and float(lo[1]) != 0.0 and float(mid[2]) == 0.0   # below 512 a multiple of 2^-8 needs two pieces at most


def test_describe_reports_position_and_values():
    a = torch.zeros(2, 4, 4, 64)
    b = a.clone()
    b[1, 2, 3, 5] = 7.0
    a[0, 0, 0, 0] = float("nan")
    msg = c6.describe(a, b)
    assert msg.startswith("2 of 2048 elements differ") and "(1, 2, 3, 5): got 0.0, expected 7.0" in msg and "(0, 0, 0, 0): got nan" in msg
