"""GPU: every plain GEMM engine and every rung of gemm_route.hip's ladder against exact references (tests/gemm_ref.py).

Each case of gemm_ref.CASES goes through lrcn_debug_gemm (include/lrcn_gemm_debug.h) -- launch_gemm on the test's own operands -- under the
router's own knobs, and first asserts the route lrcn_debug_route reports: a case that silently took another rung fails.  Integer-regime
cases are compared with np.array_equal (any f32 summation order is exact there, gemm_ref's docstring); real-valued cases against the
derived bound (K + 34) 2^-24 (|A| |B|^T + |bias| + |C0|) (+ 2^-8 |ref| for a bf16 output).  In every case C's padding columns, its guard
row behind row M - 1 and the lead-in before its first element must come back bit for bit, and the operands' padding holds 2^15, so one
element read past K, past row M or N, or before the base breaks exactness.

Route readings that the router corrected (the shapes are kept, the asserted route is what the planners give):
  * (2048, 4096, 128) without a knob is "8p:1": 128 tiles of 256 x 256 are fewer than 200 while 256 tiles of 256 x 128 are not
    (gemm_8p_config); the first no-knob "8p:0" is (2560, 5120, 128), 200 tiles.
  * (300, 512, 2048) with an f32 output is "glds", not "glds-small": gemm_glds_blocks counts the 8 K-slices, 24 x 8 = 192 >= 96.  The
    atomic split-K under "glds-small" is (300, 512, 512): 24 tiles x 2 slices.  With deterministic = 1 the split goes and both shapes
    are "glds-small".
  * (513, 1024, 128) with bg_cus = 32, one row past the 8p-bg window, is "glds-small".
  * skinny, glds, skinny-last, glds-small and gemm_nt report no ":suffix"; 8p-bg reports its tile config (":1").
PLAIN mode on the 512 x 128 tile ("8p:2") has one case, (204300, 128, 128): the tile is chosen from 400 row tiles only.
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as gr
import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu

KNOBS = ("LRCN_8P", "LRCN_GLDS", "LRCN_SKINNY", "LRCN_8P_SPLITK", "LRCN_8P_SPLITK_MIN")


@pytest.fixture(scope="module")
def ctx():
    return L.Context(8, 8, 8, 17, max_B=2, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16)   # its 48 MiB split-K workspace is production's


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run(ctx, cs, p):
    """The case on the device: (route, C's whole allocation afterwards on the host)."""
    A, B, C = p.A_flat.cuda(), p.B_flat.cuda(), p.C_flat.cuda()
    bias = p.bias.cuda() if cs.bias else None
    assert bias is None or bias.data_ptr() % 16 == 0
    route = L.debug_gemm(ctx, cs.dtype, A[p.off_ab:], B[p.off_ab:], C[p.off_c:], cs.M, cs.N, cs.K, p.lda, p.ldb, p.ldc, bias=bias,
                         c_f32=cs.c_f32, beta=cs.beta, relu=cs.relu, c_is_zero=cs.c_is_zero, deterministic=cs.det, free_cus=cs.free_cus,
                         bg_cus=cs.bg_cus, wg_cap=cs.wg_cap)
    # the operands are inputs: nothing may have written them
    assert torch.equal(A.cpu().view(torch.int16 if cs.dtype == gr.BF16 else torch.int32),
                       p.A_flat.view(torch.int16 if cs.dtype == gr.BF16 else torch.int32))
    return route, C.cpu()


def split_interior(p, flat):
    """(interior [M][N], everything else as bits with the interior blanked) of a C allocation."""
    cs = p.case
    view = flat[p.off_c:].view(cs.M + 1, p.ldc)
    interior = view[:cs.M, :cs.N].clone()
    rest = flat.clone()
    rest[p.off_c:].view(cs.M + 1, p.ldc)[:cs.M, :cs.N] = 0
    return interior, gr.bits(rest)


@pytest.mark.parametrize("cs", gr.CASES, ids=[c.id for c in gr.CASES])
def test_engine_case(ctx, monkeypatch, cs):
    p = gr.Problem(cs)
    set_knobs(monkeypatch, cs.env)
    route, got_flat = run(ctx, cs, p)
    assert route == cs.route, (cs.id, route)
    got, got_rest = split_interior(p, got_flat)
    _, want_rest = split_interior(p, p.C_flat)
    stray = np.flatnonzero(got_rest != want_rest)
    assert stray.size == 0, "%s: %d elements outside C[M][N] were written, first at flat offset %d (C starts at %d, ldc %d)" % (
        cs.id, stray.size, stray[0], p.off_c, p.ldc)
    g = got.double().numpy()
    if cs.regime == "int":
        e = p.expected.double().numpy()
        if not np.array_equal(g, e):
            r, c = np.nonzero(g != e)
            raise AssertionError("%s: %d of %d elements differ; rows %d..%d, columns %d..%d; first (%d, %d): got %r, expected %r" % (
                cs.id, r.size, g.size, r.min(), r.max(), c.min(), c.max(), r[0], c[0], g[r[0], c[0]], e[r[0], c[0]]))
        assert got.dtype == p.expected.dtype
    else:
        err = np.abs(g - p.ref)
        worst = float((err / p.bound).max())
        print("%s: worst error / bound = %.3g" % (cs.id, worst))
        assert np.isfinite(g).all() and (err <= p.bound).all(), (cs.id, worst)


# ---- refusals: gemm.h promises that the router "returns an error; never faults on bad shapes".  Each case below is rejected on the host
# before any launch, as launch_gemm_routed reads top to bottom: M <= 0 and a NULL C by its first check; a leading dimension that is not
# whole 16-byte chunks and a misaligned A fail gemm_glds_eligible (so every 8p / 8p-bg / 8p-splitk / glds rung, which all ask it) and
# gemm_skinny_eligible, and then the argument check in front of gemm_nt.
def _refusals():
    ok = dict(dtype=gr.BF16, M=64, N=64, K=64, lda=64, ldb=64, ldc=64, a_shift=0, null_c=False)
    return [
        ("lda-not-whole-chunks-bf16", dict(ok, lda=68)),
        ("lda-not-whole-chunks-f32", dict(ok, dtype=gr.F32, lda=66)),
        ("ldb-not-whole-chunks-bf16", dict(ok, M=300, N=512, K=128, lda=128, ldb=132, ldc=512)),
        ("misaligned-A", dict(ok, a_shift=4)),
        ("misaligned-A-large", dict(ok, M=300, N=512, K=128, lda=128, ldb=128, ldc=512, a_shift=4)),
        ("M-zero", dict(ok, M=0)),
        ("null-C", dict(ok, null_c=True)),
    ]


@pytest.mark.parametrize("name,r", _refusals(), ids=[n for n, _ in _refusals()])
def test_router_refuses_on_the_host_and_leaves_c_untouched(ctx, monkeypatch, name, r):
    set_knobs(monkeypatch, {})
    t = torch.float32 if r["dtype"] == gr.F32 else torch.bfloat16
    rows = max(r["M"], 1) + 1
    A = torch.ones(rows * r["lda"] + 16, dtype=t, device="cuda")
    B = torch.ones((r["N"] + 1) * r["ldb"], dtype=t, device="cuda")
    C = torch.full((rows * r["ldc"],), gr.C_SENTINEL, dtype=t, device="cuda")
    before = gr.bits(C)
    a_ptr = A.data_ptr() + r["a_shift"]
    with pytest.raises(L.LrcnError) as ei:
        L.debug_gemm(ctx, r["dtype"], a_ptr, B, None if r["null_c"] else C, r["M"], r["N"], r["K"], r["lda"], r["ldb"], r["ldc"])
    assert "error %d" % -1 in str(ei.value) and "debug_gemm" in str(ei.value), str(ei.value)   # LRCN_EINVAL with the usual message
    torch.cuda.synchronize()
    assert np.array_equal(gr.bits(C), before)


def test_null_arguments_and_unknown_dtype(ctx):
    lib = _lib.lib()
    assert lib.lrcn_debug_gemm(ctx._h, None) == -1
    assert lib.lrcn_debug_gemm(None, ctypes.byref(_lib.GemmDebug())) == -1
    C = torch.zeros(64 * 64, dtype=torch.float32, device="cuda")
    with pytest.raises(L.LrcnError):
        L.debug_gemm(ctx, _lib.LRCN_FP8, C, C, C, 64, 64, 64, 64, 64, 64)

