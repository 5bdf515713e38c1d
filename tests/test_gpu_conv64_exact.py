"""GPU: the halo-patch first-layer kernels -- conv64.hip plain and FUSE, conv64f.hip, conv11.hip -- bit for bit against tests/conv64_ref.py.

PLAIN   conv64_kernel<POOL, false> through lrcn_debug_conv64 (include/lrcn_conv_debug.h) on the test's own NHWC operands under the case's
        workgroup cap: the persistent walk (tiles b, b + G, ...), the three-patch ring (buf = j % 3, patch j + 2 issued while j is
        multiplied), the walk's tail (tile_at(j) = -1) and the launcher's cap / chunks arithmetic, none of which lrcn_conv3x3 reaches (it
        launches one workgroup per tile).  First the route ("conv64"), then nothing outside y's interior may have changed (guard row and
        lead-in bit for bit) and x and w must not have been written, then torch.equal with the expected bf16 tensor; a capped case also
        equals its uncapped run bit for bit.  x lies between margins of 2^15: a halo pixel not taken from the zero page breaks exactness.
FUSED   lrcn_conv1_fused under LRCN_FUSE11_GEN=2 (conv64f.hip) and =1 (conv64_kernel<true, true>), cap through lrcn_vgg_set_wg_cap: route
        "conv64-fused11", then torch.equal.  The one bf16 rounding between conv1_1 and conv1_2 is a round-to-nearest-even of an exactly
        known number; conv1_1's bias needs all three of its bf16 pieces in 36 channels and is positive in 54, so a conv1_1 value that
        leaks into conv1_2's zero padding is not cut by the ReLU there.
CONV11  lrcn_debug_conv11 from the uint8 crops and from the float tensor holding the same integers: torch.equal with the first stage.

Every comparison is exact because the inputs keep every partial sum inside a 24-bit window (conv64_ref's docstring: the conditions are
asserted on the host for every case); no tolerance appears anywhere in this module.  A failure reports the count and the first few (image,
y, x, channel) with got / expected.

On the MI355X every case is bit-exact: v_mfma_f32_32x32x16_bf16 (conv64f.hip's conv1_2, conv11.hip) and 16x16x32 (conv64.hip, conv64f.hip's
producer) sum these 24-bit windows exactly.

Two local builds (not kept; arithmetic only, no address or bound touched) show what the fused cases catch:
  (a) repack_conv11_w_fused_kernel writes 0 for the middle bias piece (k' = 28): all 8 test_fused_first_launch_case[*-conv64f] fail -- a
      third of the outputs, in every image and at every pixel (S16-N1: 1372 of 4096, e.g. (0, 0, 0, 0) got 9344, expected 9280; S16-N258:
      325818 of 1056768); the conv64-FUSE cases, which add b11 as an f32, pass, as do conv11 and the plain cases.
      test_gpu_vgg_parity.py::test_fused_conv1_launch_vs_emulating_oracle notices it as well: its five [*-2] cases fail at "nearly every
      value identical" (0.82 .. 0.86 identical against > 0.999), [*-1] pass.
  (b) conv64f.hip's p_set_tile leaves the px = 17 flag out of p_edge, so the produced patch's last halo column is not zeroed at the image
      border and relu(b11) enters conv1_2's padding: all 8 [*-conv64f] cases fail, and ONLY in the last pooled column (S16: x = 7, S32:
      x = 15, S48: x = 23, S224: x = 111; S224-N1: 3148 of 802816, e.g. (0, 0, 111, 6) got 0, expected 3312), in every image and
      pooled row; everything else passes.  test_fused_conv1_launch_vs_emulating_oracle notices it too: its five [*-2] cases fail at
      rel_max_err (0.12 .. 0.27 against 2e-2).
So the tolerance-based test sees both -- what it cannot do is say where, or hold the walk, the ring and the cap arithmetic of the plain kernel,
which it does not run.
"""
import ctypes

import numpy as np
import pytest
import torch

import conv64_ref as c6
import gemm_ref as gr
import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu

KNOBS = ("LRCN_CONV64", "LRCN_FUSE11", "LRCN_FUSE11_GEN", "LRCN_STAMPS", "LRCN_DYN_TILES")


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(8, 8, 8, 17, max_B=2, max_T=1, vgg_dtype=lrcn_amd.LRCN_BF16)
    yield c
    c.close()


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def equal_or_report(name, got, want):
    """torch.equal of two [n][r][q][c] tensors (a NaN is never equal), with conv64_ref.describe's report."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        raise AssertionError("%s: %s" % (name, c6.describe(got, want)))


# ------------------------------------------------------------------------------------------------------------------------------- plain
def run_plain(ctx, cs, p, wg_cap):
    """The case on the device: (route, x, w and y's whole allocations afterwards on the host)."""
    x, w, y = p.x_flat.cuda(), p.w_flat.cuda(), p.y_flat.cuda()
    bias = p.bias.cuda() if cs.bias else None
    for t in (x[p.xm:], w[p.off_w:], y[p.off_c:]):
        assert t.data_ptr() % 16 == 0
    assert x[p.xm:].data_ptr() % 4096 != 0
    route = L.debug_conv64(ctx, x[p.xm:], w[p.off_w:], y[p.off_c:], cs.N, cs.H, cs.W, cs.Cout, bias=bias, relu=cs.relu, pool=cs.pool,
                           wg_cap=wg_cap)
    return route, x.cpu(), w.cpu(), y.cpu()


def split_interior(p, flat):
    """(interior [out_rows][Cout], everything else as bits with the interior blanked) of a y allocation."""
    cs = p.case
    interior = flat[p.off_c:].view(cs.out_rows + 1, cs.ldc)[:cs.out_rows, :cs.Cout].clone()
    rest = flat.clone()
    rest[p.off_c:].view(cs.out_rows + 1, cs.ldc)[:cs.out_rows, :cs.Cout] = 0
    return interior, gr.bits(rest)


@pytest.mark.parametrize("cs", c6.PLAIN_CASES, ids=[c.id for c in c6.PLAIN_CASES])
def test_plain_conv64_case(ctx, monkeypatch, cs):
    p = c6.Problem(cs)
    set_knobs(monkeypatch, {})
    route, x_after, w_after, y_after = run_plain(ctx, cs, p, cs.wg_cap)
    assert route == "conv64" == cs.route, (cs.id, route)
    got, got_rest = split_interior(p, y_after)
    _, want_rest = split_interior(p, p.y_flat)
    stray = np.flatnonzero(got_rest != want_rest)
    assert stray.size == 0, "%s: %d elements outside y's interior were written, first at flat offset %d (y starts at %d, %d elements)" % (
        cs.id, stray.size, stray[0], p.off_c, cs.out_rows * cs.Cout)
    assert np.array_equal(gr.bits(x_after), gr.bits(p.x_flat)) and np.array_equal(gr.bits(w_after), gr.bits(p.w_flat)), cs.id
    Ho, Wo = (cs.H // 2, cs.W // 2) if cs.pool else (cs.H, cs.W)
    equal_or_report(cs.id, got.view(cs.N, Ho, Wo, cs.Cout), p.expected.view(cs.N, Ho, Wo, cs.Cout))
    if cs.wg_cap:   # the walk under the cap computes what the uncapped grid computes
        route0, _, _, y_uncapped = run_plain(ctx, cs, p, 0)
        assert route0 == "conv64", (cs.id, route0)
        diff = gr.bits(y_uncapped) != gr.bits(y_after)
        assert not diff.any(), "%s: capped and uncapped runs differ in %d elements, first at flat offset %d" % (
            cs.id, diff.sum(), np.flatnonzero(diff)[0])


def test_debug_conv64_refuses_on_the_host_and_leaves_y_untouched(ctx, monkeypatch):
    """Every refusal of include/lrcn_conv_debug.h's lrcn_debug_conv64: LRCN_EINVAL before any launch, y bit for bit as it was."""
    set_knobs(monkeypatch, {})
    lib = _lib.lib()
    x = torch.ones(2 * 16 * 16 * 64 + 16, dtype=torch.bfloat16, device="cuda")
    w = torch.ones(64 * 9 * 64 + 16, dtype=torch.bfloat16, device="cuda")
    y = torch.full((2 * 16 * 16 * 64 + 16,), gr.C_SENTINEL, dtype=torch.bfloat16, device="cuda")
    before = gr.bits(y)
    px, pw, py = x.data_ptr(), w.data_ptr(), y.data_ptr()
    assert px % 16 == 0 and pw % 16 == 0 and py % 16 == 0

    def call(handle, x=px, w=pw, y=py, N=2, H=16, W=16, Cout=64):
        d = _lib.Conv64Debug(x, w, None, y, N, H, W, Cout, 0, 0, 0)
        return lib.lrcn_debug_conv64(handle, ctypes.byref(d))

    assert call(ctx._h) == 0   # the arguments every refusal below departs from are accepted
    y.fill_(gr.C_SENTINEL)
    torch.cuda.synchronize()
    refused = {
        "x NULL": dict(x=None), "w NULL": dict(w=None), "y NULL": dict(y=None),
        "W % 16": dict(W=24), "H % 16": dict(H=8), "W < 16": dict(W=0), "Cout % 64": dict(Cout=96), "Cout < 64": dict(Cout=0),
        "N < 1": dict(N=0), "N < 0": dict(N=-1),
        "N * H * W * 64 = 2^31": dict(N=2 ** 31 // (16 * 16 * 64)),
        "x misaligned": dict(x=px + 8), "w misaligned": dict(w=pw + 2), "y misaligned": dict(y=py + 8),
    }
    for name, k in refused.items():
        assert call(ctx._h, **k) == -1, name
    assert lib.lrcn_debug_conv64(ctx._h, None) == -1
    assert call(None) == -1
    f32 = L.Context(8, 8, 8, 17, max_B=2, max_T=1, vgg_dtype=lrcn_amd.LRCN_F32)   # the f32 stack has no conv64.hip
    assert call(f32._h) == -1
    f32.close()
    torch.cuda.synchronize()
    assert np.array_equal(gr.bits(y), before)
    with pytest.raises(L.LrcnError) as ei:   # through the wrapper: LRCN_EINVAL with the usual message
        L.debug_conv64(ctx, x, w, y, 2, 16, 24, 64)
    assert "error %d" % -1 in str(ei.value) and "debug_conv64" in str(ei.value), str(ei.value)
    torch.cuda.synchronize()
    assert np.array_equal(gr.bits(y), before)


# ------------------------------------------------------------------------------------------------------------------------------- fused
@pytest.mark.parametrize("gen", ["2", "1"], ids=["conv64f", "conv64-FUSE"])
@pytest.mark.parametrize("key", c6.FUSED_CASES, ids=["S%d-N%d-cap%d" % k for k in c6.FUSED_CASES])
def test_fused_first_launch_case(ctx, monkeypatch, key, gen):
    S, N, cap = key
    f = c6.fused(S, N)
    s = f.s1
    set_knobs(monkeypatch, {"LRCN_FUSE11_GEN": gen})
    L.vgg_set_wg_cap(ctx, cap)
    try:
        y = L.conv1_fused(ctx, s.img.cuda(), c6.MEAN, L.to_jl(c6.to_ref_w(s.w11).float().numpy()), s.b11.float().cuda(),
                          L.to_jl(c6.to_ref_w(f.w12).float().numpy()), f.b12.float().cuda())
        route = L.debug_route(ctx)
    finally:
        L.vgg_set_wg_cap(ctx, 0)
    assert route == "conv64-fused11", (key, gen, route)
    got = c6.from_ref_y(L.from_jl(y))   # f32 holding the kernel's bf16 values, [n][r][q][co]
    equal_or_report("fused S=%d N=%d cap=%d gen=%s" % (S, N, cap, gen), got, f.expected.float())


# ------------------------------------------------------------------------------------------------------------------------------ conv11
@pytest.mark.parametrize("S,N", c6.CONV11_CASES)
def test_conv11_case(ctx, monkeypatch, S, N):
    s = c6.stage1(S, N)
    set_knobs(monkeypatch, {})
    w, b = L.to_jl(c6.to_ref_w(s.w11).float().numpy()), s.b11.float().cuda()
    got8 = c6.from_ref_y(L.from_jl(L.debug_conv11(ctx, s.img.cuda(), w, b, mean=c6.MEAN)))
    gotf = c6.from_ref_y(L.from_jl(L.debug_conv11(ctx, L.to_jl(c6.to_ref_x(s.x).float().numpy()), w, b)))
    equal_or_report("conv11 uint8 source S=%d N=%d" % (S, N), got8, s.a1.float())
    equal_or_report("conv11 float source S=%d N=%d" % (S, N), gotf, s.a1.float())
