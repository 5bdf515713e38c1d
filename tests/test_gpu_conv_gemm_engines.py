"""GPU: the convolution (CONV3) operand mode of every GEMM engine and router rung against exact references (tests/conv_gemm_ref.py).

Each case of conv_gemm_ref.CASES goes through lrcn_debug_conv_gemm (include/lrcn_gemm_debug.h) -- launch_gemm in CONV3 mode on the test's
own NHWC operands, never conv64.hip -- under the router's own knobs, and FIRST asserts the route lrcn_debug_route reports: a case that
silently took another rung fails.  Then nothing outside y's interior may have changed (padding columns, guard row and lead-in come back bit
for bit) and x and w must not have been written.  Then the values: integer-regime cases with np.array_equal (any f32 summation order is
exact there, conv_gemm_ref's docstring), real-valued cases against the derived bound (9 Cin + 34) 2^-24 (|x| * |w| + |bias|) (+ 2^-8 |ref|
for a bf16 output; the largest of a pool window's four).  x sits between margins of 2^15 as long as the taps of the first and last image
rows reach, so a wrong border mask breaks exactness.  A capped case (wg_cap: the persistent walk of gemm8p_kernel, tiles w, w + G, ...) also
equals its uncapped run bit for bit.

Route readings that the router corrected (the shapes are kept, the asserted route is what the planners give):
  * 16 x 16 x 4 images, 512 -> 512 with LRCN_8P_SPLITK=0 is "glds-small", not "glds": choose_cfg's best grid is 64 tiles of 128 x 64,
    fewer than the 96 that "glds" asks for without LRCN_GLDS=force.
  * 14 x 14 x 2 images, 192 -> 136 has Cout % 8 == 0; the reduce kernel's Cout % 8 != 0 (and W != H under split-K) is the added case
    12 x 20 x 2 images, 192 -> 132.
The glds and gemm_nt route strings do not carry the tile; each case's tag states the tile that choose_cfg (gemm_glds.hip) / dispatch
(gemm.hip) pick for its shape: glds 16 x 16 x 100 images -> 512 / 256 / 128 channels are 200 workgroups of 256 x 256 / 256 x 128 / 256 x 64,
720-row cases 128 x 64; gemm_nt takes 128 x 128 tiles from 160 of them (16 x 16 x 40 images -> 256: exactly 160).

The last block runs three of the same integer problems through the ABI's lrcn_conv3x3 in the reference's layouts, which adds
k_ref_to_nhwc, k_repack_conv_w (with their channel padding) and k_nhwc_to_ref -- the layout kernels lrcn_debug_conv_gemm bypasses.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv_gemm_ref as cr
import gemm_ref as gr
import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu

KNOBS = ("LRCN_8P", "LRCN_GLDS", "LRCN_SKINNY", "LRCN_8P_SPLITK", "LRCN_8P_SPLITK_MIN", "LRCN_CONV64")


@pytest.fixture(scope="module")
def ctx():
    return L.Context(8, 8, 8, 17, max_B=2, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16)   # its 48 MiB split-K workspace is production's


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run(ctx, cs, p, wg_cap):
    """The case on the device: (route, x, w and y's whole allocations afterwards on the host)."""
    x, w, y = p.x_flat.cuda(), p.w_flat.cuda(), p.y_flat.cuda()
    bias = p.bias.cuda() if cs.bias else None
    assert bias is None or bias.data_ptr() % 16 == 0
    assert x[p.xm:].data_ptr() % 16 == 0 and x[p.xm:].data_ptr() % 4096 != 0
    route = L.debug_conv_gemm(ctx, cs.dtype, x[p.xm:], w[p.off_w:], y[p.off_c:], cs.N, cs.H, cs.W, cs.Cin, cs.Cout, cs.ldc, bias=bias,
                              relu=cs.relu, pool=cs.pool, wg_cap=wg_cap)
    return route, x.cpu(), w.cpu(), y.cpu()


def split_interior(p, flat):
    """(interior [out_rows][Cout], everything else as bits with the interior blanked) of a y allocation."""
    cs = p.case
    interior = flat[p.off_c:].view(cs.out_rows + 1, cs.ldc)[:cs.out_rows, :cs.Cout].clone()
    rest = flat.clone()
    rest[p.off_c:].view(cs.out_rows + 1, cs.ldc)[:cs.out_rows, :cs.Cout] = 0
    return interior, gr.bits(rest)


def describe(cs, bad):
    """Where a boolean [out_rows][Cout] mask is set: counts, ranges and the images, rows and columns of the pixels."""
    r, c = np.nonzero(bad)
    n, y, x = cr.where(cs, r)
    return "%d of %d elements; output rows %d..%d, channels %d..%d (distinct %d); images %s; pixel rows %s; pixel columns %s" % (
        r.size, bad.size, r.min(), r.max(), c.min(), c.max(), np.unique(c).size, np.unique(n)[:12].tolist(), np.unique(y).tolist(),
        np.unique(x).tolist())


def check_values(cs, p, got):
    g = got.double().numpy()
    if cs.regime == "int":
        e = p.expected.double().numpy()
        if not np.array_equal(g, e):
            r, c = np.nonzero(g != e)
            raise AssertionError("%s: %s; first (%d, %d): got %r, expected %r" % (cs.id, describe(cs, g != e), r[0], c[0], g[r[0], c[0]],
                                                                                 e[r[0], c[0]]))
        assert got.dtype == p.expected.dtype
    else:
        err = np.abs(g - p.ref)
        worst = float((err / p.bound).max())
        print("%s: worst error / bound = %.3g" % (cs.id, worst))
        bad = ~(err <= p.bound)   # a NaN is bad too
        assert not bad.any(), "%s: worst error / bound = %.3g; %s" % (cs.id, worst, describe(cs, bad))


@pytest.mark.parametrize("cs", cr.CASES, ids=[c.id for c in cr.CASES])
def test_conv_engine_case(ctx, monkeypatch, cs):
    p = cr.Problem(cs)
    set_knobs(monkeypatch, cs.env)
    route, x_after, w_after, y_after = run(ctx, cs, p, cs.wg_cap)
    assert route == cs.route, (cs.id, route)
    got, got_rest = split_interior(p, y_after)
    _, want_rest = split_interior(p, p.y_flat)
    stray = np.flatnonzero(got_rest != want_rest)
    assert stray.size == 0, "%s: %d elements outside y's interior were written, first at flat offset %d (y starts at %d, ldc %d)" % (
        cs.id, stray.size, stray[0], p.off_c, cs.ldc)
    # the operands are inputs: nothing may have written them
    assert np.array_equal(gr.bits(x_after), gr.bits(p.x_flat)) and np.array_equal(gr.bits(w_after), gr.bits(p.w_flat)), cs.id
    check_values(cs, p, got)
    if cs.wg_cap:   # the walk under the cap computes what one workgroup per tile computes
        route0, _, _, y_uncapped = run(ctx, cs, p, 0)
        assert route0 == cs.route, (cs.id, route0)
        diff = gr.bits(y_uncapped) != gr.bits(y_after)
        assert not diff.any(), "%s: capped and uncapped runs differ in %d elements, first at flat offset %d" % (
            cs.id, diff.sum(), np.flatnonzero(diff)[0])


# ---- refusals: gemm.h promises that the router "returns an error; never faults on bad shapes".  Each case below is rejected on the host
# before any launch: a bf16 Cin that is no multiple of 64, an odd W and a misaligned x fail gemm_glds_eligible (so every 8p / 8p-splitk /
# glds rung, which all ask it) and then the argument check in front of gemm_nt; a NULL y fails launch_gemm_routed's first check; N = 0 and
# an element type other than f32 / bf16 never leave the entry.
def _refusals():
    ok = dict(dtype=gr.BF16, N=2, H=8, W=8, Cin=64, Cout=64, x_shift=0, null_y=False)
    return [
        ("bf16-Cin-48", dict(ok, Cin=48)),
        ("odd-W", dict(ok, W=7)),
        ("misaligned-x", dict(ok, x_shift=4)),
        ("null-y", dict(ok, null_y=True)),
        ("N-zero", dict(ok, N=0)),
        ("dtype-fp8", dict(ok, dtype=_lib.LRCN_FP8)),
    ]


@pytest.mark.parametrize("name,r", _refusals(), ids=[n for n, _ in _refusals()])
def test_router_refuses_on_the_host_and_leaves_y_untouched(ctx, monkeypatch, name, r):
    set_knobs(monkeypatch, {})
    n = max(r["N"], 1)
    margin = (r["W"] + 1) * r["Cin"] + 64
    x = torch.ones(2 * margin + n * r["H"] * r["W"] * r["Cin"] + 16, dtype=torch.bfloat16, device="cuda")
    w = torch.ones((r["Cout"] + 1) * 9 * r["Cin"], dtype=torch.bfloat16, device="cuda")
    y = torch.full(((n * r["H"] * r["W"] + 1) * r["Cout"],), gr.C_SENTINEL, dtype=torch.bfloat16, device="cuda")
    before = gr.bits(y)
    x_ptr = x[margin // 8 * 8:].data_ptr() + r["x_shift"]
    with pytest.raises(L.LrcnError) as ei:
        L.debug_conv_gemm(ctx, r["dtype"], x_ptr, w, None if r["null_y"] else y, r["N"], r["H"], r["W"], r["Cin"], r["Cout"], r["Cout"])
    assert "error %d" % -1 in str(ei.value) and "debug_conv_gemm" in str(ei.value), str(ei.value)   # LRCN_EINVAL with the usual message
    torch.cuda.synchronize()
    assert np.array_equal(gr.bits(y), before)


def test_null_arguments(ctx):
    lib = _lib.lib()
    assert lib.lrcn_debug_conv_gemm(ctx._h, None) == -1
    assert lib.lrcn_debug_conv_gemm(None, ctypes.byref(_lib.ConvGemmDebug())) == -1


# ---- the same integer problems through the ABI entry: reference layouts in, k_ref_to_nhwc / k_repack_conv_w (channels padded to the
# engines' K-tile) / the routed engine / k_nhwc_to_ref, reference layout out, against the same exact reference
ABI_CASES = [
    cr.Case("conv64", 16, 16, 3, 64, 128, dtype=gr.BF16),        # the halo-patch kernel of the Cin = 64 layers
    cr.Case("glds-small", 12, 20, 3, 96, 136, dtype=gr.BF16),    # channels padded 96 -> 128: 18 tiles of 128 x 64
    cr.Case("glds-small", 12, 20, 3, 40, 136, dtype=gr.F32),     # channels padded 40 -> 64
]


@pytest.fixture(scope="module")
def abi_ctx():
    return {t: L.Context(8, 8, 8, 17, max_B=2, max_T=1, vgg_dtype=t) for t in (lrcn_amd.LRCN_BF16, lrcn_amd.LRCN_F32)}


@pytest.mark.parametrize("relu_pool", [False, True], ids=["plain", "relu-pool"])
@pytest.mark.parametrize("base", ABI_CASES, ids=[c.id for c in ABI_CASES])
def test_abi_conv3x3_is_exact_in_the_reference_layouts(abi_ctx, monkeypatch, base, relu_pool):
    cs = cr.Case(base.route, base.W, base.H, base.N, base.Cin, base.Cout, dtype=base.dtype, relu=relu_pool, pool=relu_pool)
    p = cr.Problem(cs)
    set_knobs(monkeypatch, {})
    ctx = abi_ctx[lrcn_amd.LRCN_BF16 if cs.dtype == gr.BF16 else lrcn_amd.LRCN_F32]
    x = L.to_jl(p.x.float().permute(2, 1, 3, 0))                                                   # (W, H, Cin, N)
    w = L.to_jl(p.w[:cs.Cout].float().reshape(cs.Cout, 3, 3, cs.Cin).permute(2, 1, 3, 0))          # (kw, kh, Cin, Cout)
    b = (p.bias if cs.bias else torch.zeros(cs.Cout)).cuda()
    y = L.from_jl(L.conv3x3(ctx, x, w, b, relu=cs.relu, pool=cs.pool))                             # (Wo, Ho, Cout, N)
    assert L.debug_route(ctx) == cs.route, (cs.id, L.debug_route(ctx))
    got = torch.from_numpy(np.ascontiguousarray(y.transpose(3, 1, 0, 2))).reshape(cs.out_rows, cs.Cout)
    e = p.expected.float()   # the bf16 stack's output widens to f32 exactly
    if not torch.equal(got, e):
        bad = (got != e).numpy()
        raise AssertionError("%s through lrcn_conv3x3: %s" % (cs.id, describe(cs, bad)))
