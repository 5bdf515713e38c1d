"""CPU: the host references of tests/fp8_ref.py against each other -- torch's float8_e4m3fn cast and the written-out round-half-even agree
on every bf16 bit pattern at every factor the GPU cast tests use, and the byte decoding is the format's."""
import numpy as np
import pytest
import torch

import fp8_ref as F


@pytest.mark.parametrize("factor", F.FACTORS)
def test_torch_cast_and_written_out_rounding_agree_on_every_bf16_pattern(factor):
    x = F.all_bf16_patterns()          # NaN patterns -> 0; +-inf, +-0 and every subnormal kept
    assert x.numel() == 65536 and bool(torch.isinf(x).sum() == 2) and not bool(torch.isnan(x).any())
    v = F.scaled(x, factor)
    a, b = F.e4m3(v), F.e4m3_rne_numpy(v)
    assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)), int((a != b).sum())
    assert np.abs(a).max() == 448.0 and a[x.float().numpy() == np.inf][0] == 448.0 and a[x.float().numpy() == -np.inf][0] == -448.0
    # the bytes are those values
    assert np.array_equal(F.from_e4m3_bytes(F.e4m3_bytes(v)), a)
    assert np.array_equal(np.signbit(F.from_e4m3_bytes(F.e4m3_bytes(v))), np.signbit(a))


def test_byte_decoding_is_the_formats():
    d = F.from_e4m3_bytes(np.array([0x7F, 0xFF, 0x7E, 0x01, 0xFE, 0x80, 0x08, 0x38], np.uint8))
    assert np.isnan(d[0]) and np.isnan(d[1])
    assert d[2] == 448.0 and d[3] == 2.0 ** -9 and d[4] == -448.0 and d[5] == 0.0 and np.signbit(d[5]) and d[6] == 2.0 ** -6 and d[7] == 1.0
    every = np.arange(256, dtype=np.uint8)
    t = torch.as_tensor(every).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    mine = F.from_e4m3_bytes(every)
    assert np.array_equal(np.isnan(t), np.isnan(mine)) and np.isnan(mine).sum() == 2
    ok = ~np.isnan(t)
    assert np.array_equal(t[ok], mine[ok]) and np.array_equal(np.signbit(t[ok]), np.signbit(mine[ok]))
    # every finite byte survives value -> byte -> value
    assert np.array_equal(F.e4m3_bytes(mine[ok]), every[ok])


@pytest.mark.parametrize("W,H,Cout,N,cap", F.CONV64_CASES)
def test_conv64_epilogue_emulation_does_not_depend_on_how_the_host_sums(W, H, Cout, N, cap):
    """The cap test_gpu_fp8_seams.py puts on conv2_1's e4m3 epilogue (>= 99 % of the values identical to the float64 emulation) is far from
    what summation order alone does: the same emulation from sums made another way differs in under 0.1 % of the values at every shape and
    both scales.  Counts of differing values (non-saturating / saturating scale), of 16384, 589824, 360448 and 294912 values:
    torch conv2d accumulating in float32 -- 0/0, 0/0, 1/0, 2/1; the CPU oracle's conv3x3 (double sum rounded once to float32) -- 0 everywhere.
    Also the operands' own preconditions: the 4x scale saturates between 1 % and 50 % of the tensor, the 1x scale clamps nothing."""
    from oracle import oracle as orc
    x, w, b = F.conv64_case(W, H, Cout, N)
    acc = F.conv3x3_relu(x, w, b)
    acc32 = F.conv3x3_relu(x, w, b, dtype=torch.float32)
    acco = orc.conv3x3(F.bf16_round(x, torch.float32).numpy(), F.bf16_round(w, torch.float32).numpy(), b, relu=True)
    assert acc.shape == acco.shape == (W, H, Cout, N) and (acc == 0).any()
    inv = np.float32(448.0) / np.float32(acc.max())
    for k in (1, 4):
        emu = F.conv64_f8_emulation(acc, np.float32(k) * inv)
        sat = float((emu == 448.0).mean())
        assert (0.01 <= sat <= 0.5) if k == 4 else (0 < sat < 0.01), (k, sat)   # x1: only values that ROUND to 448, none clamped
        for name, other in (("float32 conv2d", acc32), ("oracle conv3x3", acco)):
            n = int((F.conv64_f8_emulation(other, np.float32(k) * inv) != emu).sum())
            print("%s x%d: %d of %d differ" % (name, k, n, emu.size))
            assert n < 1e-3 * emu.size, (name, k, n)


def test_bf16_cast_reference_round_trips_every_byte():
    every = np.arange(256, dtype=np.uint8)
    bits = F.cast_fp8_bf16_ref(every, 1.0)      # e4m3 has 3 mantissa bits, bf16 7: exact
    back = torch.as_tensor(bits).view(torch.bfloat16)
    ok = ~np.isnan(F.from_e4m3_bytes(every))
    assert np.array_equal(F.cast_bf16_fp8_ref(back[torch.as_tensor(ok)], 1.0), every[ok])
    assert bool(torch.isnan(back[0x7F])) and bool(torch.isnan(back[0xFF]))
