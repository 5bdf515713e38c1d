"""CPU: the references and the case table of the plain GEMM engine tests (tests/gemm_ref.py) are right before any kernel is judged by them.

Every case of the table is built here, which asserts its input conditions (integer regime: K max|a| max|b| + max|bias| + max|C0| < 2^24,
both signs before the ReLU, at least half of the expected values above 2^8 and some above 2^11).  Both references are then held against a
plain torch CPU matmul of the same operands: the integer one must equal an f32 torch matmul exactly (the very claim the GPU test rests
on: any f32 summation order is exact), the real-valued one must agree with a float64 torch matmul to float64 rounding, and an f32 torch
matmul -- some f32 summation order -- must lie inside the derived bound.
"""
import re

import numpy as np
import pytest
import torch

import gemm_ref as gr
from lrcn_amd import _lib

SMALL_ENOUGH = 64 << 20   # M N K of the cases whose torch matmul is repeated here; the larger ones are checked by construction only


def test_table_covers_every_rung_twice():
    ids = [c.id for c in gr.CASES]
    assert len(ids) == len(set(ids)), "two cases share an id"
    assert 60 <= len(ids) <= 80, len(ids)
    for rung in gr.RUNGS:
        n = sum(1 for c in gr.CASES if c.route == rung or c.route.startswith(rung + ":"))
        assert n >= (1 if rung == "8p:2" else 2), (rung, n)
    assert all(c.route.split(":")[0] in {r.split(":")[0] for r in gr.RUNGS} for c in gr.CASES)
    assert sum(1 for c in gr.CASES if c.regime == "real") >= 6


def test_layout_has_padding_guard_and_lead_in():
    cs = next(c for c in gr.CASES if c.pad_a and c.pad_b and c.pad_c and c.off)
    p = gr.Problem(cs)
    assert p.lda > cs.K and p.ldb > cs.K and p.ldc > cs.N and p.lda % gr.chunk(cs.dtype) == 0
    assert p.A.shape == (cs.M + 1, p.lda) and p.C.shape == (cs.M + 1, p.ldc)
    assert (p.A[:, cs.K:] == gr.OPERAND_PAD).all() and (p.A[cs.M] == gr.OPERAND_PAD).all() and (p.A_flat[:p.off_ab] == gr.OPERAND_PAD).all()
    assert (p.B[:, cs.K:] == gr.OPERAND_PAD).all() and (p.B[cs.N] == gr.OPERAND_PAD).all()
    assert (p.C[:, cs.N:] == gr.C_SENTINEL).all() and (p.C[cs.M] == gr.C_SENTINEL).all() and (p.C_flat[:p.off_c] == gr.C_SENTINEL).all()
    assert (p.A_flat[p.off_ab:].data_ptr() - p.A_flat.data_ptr()) % 16 == 0 and p.off_ab > 0
    # the values are exact in the element type: 2^15 and the sentinel survive bf16
    assert float(torch.tensor(gr.OPERAND_PAD).bfloat16()) == gr.OPERAND_PAD and float(torch.tensor(gr.C_SENTINEL).bfloat16()) == gr.C_SENTINEL


@pytest.mark.parametrize("cs", gr.CASES, ids=[c.id for c in gr.CASES])
def test_case_conditions_and_reference_vs_torch_matmul(cs):
    p = gr.Problem(cs)   # asserts the input conditions of an integer-regime case
    if cs.M * cs.N * cs.K > SMALL_ENOUGH:
        return
    M, N, K = cs.M, cs.N, cs.K
    A, B = p.A[:M, :K], p.B[:N, :K]
    extra = torch.zeros(M, N, dtype=torch.float64)
    if cs.bias:
        extra += p.bias.double()[None, :]
    if cs.beta:
        extra += p.C[:M, :N].double()
    t32 = (A.float() @ B.float().T).double() + extra
    if cs.relu:
        t32 = t32.clamp_min(0.0)
    if cs.regime == "int":
        t32 = t32.float()
        want = t32 if cs.c_f32 else t32.bfloat16()
        assert want.dtype == p.expected.dtype and np.array_equal(gr.bits(want), gr.bits(p.expected))
        if not cs.c_f32:   # the bf16 rounding is a real one for these magnitudes: the table can tell a truncation from a rounding
            assert (p.expected.float() != t32).any()
    else:
        t64 = A.double() @ B.double().T + extra
        if cs.relu:
            t64 = t64.clamp_min(0.0)
        assert np.abs(t64.numpy() - p.ref).max() <= 1e-12 * np.abs(p.ref).max()
        got = t32.numpy() if cs.c_f32 else t32.float().bfloat16().double().numpy()
        assert (np.abs(got - p.ref) <= p.bound).all()


def test_integer_conditions_reject_small_magnitudes():
    cs = gr.Case("gemm_nt", 64, 64, 64, amax=2)   # results of a few units: exact in bf16, would prove nothing
    with pytest.raises(AssertionError):
        gr.Problem(cs)


def test_binding_declares_exactly_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.GEMM_DEBUG_HEADER).read(), flags=re.S)
    names = ["lrcn_debug_conv_gemm", "lrcn_debug_gemm"]
    assert sorted(set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt))) == sorted(_lib.GEMM_DEBUG_SIGNATURES) == names
    for name in names:
        assert name not in _lib.SIGNATURES and name not in open(_lib.HEADER).read()
