"""GPU: the HIP VGG-16 path (implicit-GEMM 3x3 conv + bias + ReLU + fused 2x2 max-pool, fc6/fc7, preprocessing) through
the C ABI against the golden vectors and the CPU oracle.  fp32: exact-fp32 MFMA, tolerance 1e-4 relative to the
tensor's max; bf16: 3e-2 relative to the tensor's max (operands rounded to 8 bits of mantissa per layer)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import lrcn as L
from oracle import oracle as orc

from fp8_ref import e4m3 as _e4m3

pytestmark = pytest.mark.gpu


def rel_max_err(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def assert_bf16_layer(got, emu, what=""):
    """A bf16 layer against the bf16-EMULATING oracle (bf16 operands, exact accumulation from the f32 bias, ReLU, one rounding to
    bf16; lrcn_oracle.h): the kernel sums in f32 in another order, so a value may land on the neighbouring bf16 (one step = at most
    2^-7 relative) when the exact sum sits at a rounding boundary -- never further, and only for a small fraction of the tensor."""
    diff = np.abs(got - emu)
    mx = np.abs(emu).max()
    assert (diff <= 2.0 ** -7 * np.abs(emu) + 1e-5 * mx).all(), (what, float(diff.max()), float(mx))
    assert (diff == 0).mean() > 0.97, (what, float((diff == 0).mean()))


def emulated_layer(x, w, b):
    with orc.emulate_bf16():
        ref = orc.conv3x3(x, w, b, relu=True)
        return ref, orc.pool2(ref), orc.conv3x3(x, w, b, relu=False)


def small_ctx(vgg_dtype=lrcn_amd.LRCN_F32, max_images=0):
    return L.Context(8, 8, 8, 17, max_B=2, max_T=1, vgg_dtype=vgg_dtype, max_images=max_images)


def test_conv_pool_vs_golden_fp32(golden_dir):
    z = np.load(os.path.join(golden_dir, "cnn_small.npz"))
    ctx = small_ctx()
    x, w, b = L.to_jl(z["x"]), L.to_jl(z["w"]), torch.as_tensor(z["b"]).cuda()
    y = L.from_jl(L.conv3x3(ctx, x, w, b, relu=True, pool=False))
    np.testing.assert_allclose(y, z["y"], rtol=1e-5, atol=1e-5)
    yp = L.from_jl(L.conv3x3(ctx, x, w, b, relu=True, pool=True))
    np.testing.assert_allclose(yp, z["yp"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("glds", ["0", "force"])
@pytest.mark.parametrize("dtype,tol", [(lrcn_amd.LRCN_F32, 1e-5), (lrcn_amd.LRCN_BF16, 2e-2)])
@pytest.mark.parametrize("shape", [(28, 64, 128, 3), (14, 128, 64, 5), (8, 96, 40, 2), (2, 32, 32, 1), (16, 64, 320, 3),
                                   (12, 192, 64, 2)])
def test_conv_layers_vs_oracle(dtype, tol, shape, glds, monkeypatch):
    # glds: the bf16 direct-to-LDS kernel (gemm_glds.hip) forced on / off; both must agree with the oracle
    monkeypatch.setenv("LRCN_GLDS", glds)
    S, Cin, Cout, N = shape
    rng = np.random.default_rng(S * 1000 + Cin)
    x = rng.standard_normal((S, S, Cin, N)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ctx = small_ctx(dtype)
    ref = orc.conv3x3(x, w, b, relu=True)
    got = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=True, pool=False))
    assert rel_max_err(got, ref) <= tol
    refp = orc.pool2(ref)
    gotp = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=True, pool=True))
    assert rel_max_err(gotp, refp) <= tol
    # no-ReLU path keeps negatives (fc7-style)
    ref_lin = orc.conv3x3(x, w, b, relu=False)
    got_lin = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=False, pool=False))
    assert (got_lin < 0).any() and rel_max_err(got_lin, ref_lin) <= tol
    if dtype == lrcn_amd.LRCN_BF16:  # the tight check: the same arithmetic with bf16 rounding, value by value
        e, ep, el = emulated_layer(x, w, b)
        assert_bf16_layer(got, e, "relu")
        assert_bf16_layer(gotp, ep, "relu + pool")
        assert_bf16_layer(got_lin, el, "linear")


@pytest.mark.parametrize("shape", [(16, 64, 256, 2), (28, 64, 128, 3), (12, 128, 136, 3), (10, 64, 384, 5), (8, 192, 512, 9),
                                   (6, 64, 200, 8)])
def test_conv_phase_interleaved_kernel_vs_oracle(shape, monkeypatch):
    # gemm_8p.hip (256x256 / 256x128 tiles, 16x16x32 MFMA, two staggered wave groups) forced on even for small grids:
    # full / partial M tiles, N tails, both epilogues (swapped plain, fused pool); and the same layer with the kernel off.
    S, Cin, Cout, N = shape
    rng = np.random.default_rng(S * 77 + Cout)
    x = rng.standard_normal((S, S, Cin, N)).astype(np.float32)
    w = (rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ref = orc.conv3x3(x, w, b, relu=True)
    refp = orc.pool2(ref)
    ref_lin = orc.conv3x3(x, w, b, relu=False)
    emu = emulated_layer(x, w, b)
    outs = {}
    for knob in ("force", "0"):
        monkeypatch.setenv("LRCN_8P", knob)
        ctx = small_ctx(lrcn_amd.LRCN_BF16)
        got = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=True, pool=False))
        gotp = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=True, pool=True))
        got_lin = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=False, pool=False))
        assert rel_max_err(got, ref) <= 2e-2 and rel_max_err(gotp, refp) <= 2e-2 and rel_max_err(got_lin, ref_lin) <= 2e-2
        for g_, e_, what in zip((got, gotp, got_lin), emu, ("relu", "relu + pool", "linear")):
            assert_bf16_layer(g_, e_, "LRCN_8P=%s %s" % (knob, what))
        outs[knob] = (got, gotp, got_lin)
        ctx.close()
    # same bf16 operands, f32 accumulation in a different order: the two kernels agree to bf16 output rounding
    for a, c in zip(outs["force"], outs["0"]):
        assert rel_max_err(a, c) <= 1e-2


@pytest.mark.parametrize("shape", [(16, 16, 64, 3), (32, 32, 128, 2), (48, 16, 64, 5), (16, 64, 192, 1), (32, 32, 64, 11)])
def test_conv64_halo_patch_kernel_vs_oracle(shape, monkeypatch):
    # conv64.hip (Cin = 64: 18x18 halo patch in LDS, weights register-resident, persistent tiles, 3 patch buffers):
    # image borders, tile borders inside an image, several 64-channel chunks, more tiles than one pass of the ring
    # (N = 11 -> 44 tiles), W != H; against the oracle and against the implicit-GEMM kernels on the same operands.
    W, H, Cout, N = shape
    rng = np.random.default_rng(W * 31 + H + Cout)
    x = rng.standard_normal((W, H, 64, N)).astype(np.float32)
    w = (rng.standard_normal((3, 3, 64, Cout)) * np.sqrt(2.0 / (9 * 64))).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    ref = orc.conv3x3(x, w, b, relu=True)
    refp = orc.pool2(ref)
    ref_lin = orc.conv3x3(x, w, b, relu=False)
    emu = emulated_layer(x, w, b)
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("LRCN_CONV64", knob)
        ctx = small_ctx(lrcn_amd.LRCN_BF16)
        got = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=True, pool=False))
        gotp = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=True, pool=True))
        got_lin = L.from_jl(L.conv3x3(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), relu=False, pool=False))
        assert rel_max_err(got, ref) <= 2e-2 and rel_max_err(gotp, refp) <= 2e-2 and rel_max_err(got_lin, ref_lin) <= 2e-2
        for g_, e_, what in zip((got, gotp, got_lin), emu, ("relu", "relu + pool", "linear")):
            assert_bf16_layer(g_, e_, "LRCN_CONV64=%s %s" % (knob, what))
        outs[knob] = (got, gotp, got_lin)
        ctx.close()
    for a, c in zip(outs["1"], outs["0"]):
        assert rel_max_err(a, c) <= 1e-2


def test_preprocess_u8_bit_exact():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(3, 224, 224, 3), dtype=np.uint8)
    ctx = small_ctx()
    got = L.from_jl(L.read_image_data_u8(ctx, torch.as_tensor(img).cuda()))
    ref = orc.preprocess_u8(img, np.array(L.VGG_MEAN, np.float32))
    np.testing.assert_array_equal(got, ref)


@pytest.fixture(scope="module")
def vgg_setup():
    w = L.synthetic_vgg_weights(seed=1)
    host = ([L.from_jl(t) for t in w[0]], [t.cpu().numpy() for t in w[1]], (L.from_jl(w[2][0]), w[2][1].cpu().numpy()),
            (L.from_jl(w[3][0]), w[3][1].cpu().numpy()))
    rng = np.random.default_rng(1234)
    img = rng.integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    x = orc.preprocess_u8(img, np.array(L.VGG_MEAN, np.float32))
    ref = orc.vgg_forward(host[0], host[1], host[2], host[3], x)  # N x 4096
    return w, img, x, ref


def test_full_vgg_fp32_vs_oracle(vgg_setup):
    w, img, x, ref = vgg_setup
    ctx = small_ctx(lrcn_amd.LRCN_F32, max_images=2)
    L.vgg_load(ctx, *w)
    got = L.from_jl(L.convnet(ctx, L.to_jl(x)))
    assert got.shape == (2, 4096) and (got < 0).any()  # pre-ReLU fc7
    assert rel_max_err(got, ref) <= 1e-4
    got8 = L.from_jl(L.convnet_u8(ctx, torch.as_tensor(img).cuda()))
    np.testing.assert_allclose(got8, got, rtol=0, atol=1e-6 * np.abs(ref).max())
    # batch of one image gives the same row (M-edge tiles)
    got1 = L.from_jl(L.convnet_u8(ctx, torch.as_tensor(img[1:2]).cuda()))
    np.testing.assert_allclose(got1[0], got8[1], rtol=0, atol=1e-5 * np.abs(ref).max())


def test_full_vgg_bf16_vs_oracle(vgg_setup):
    w, img, x, ref = vgg_setup
    ctx = small_ctx(lrcn_amd.LRCN_BF16, max_images=2)
    L.vgg_load(ctx, *w)
    got = L.from_jl(L.convnet_u8(ctx, torch.as_tensor(img).cuda()))
    assert rel_max_err(got, ref) <= 3e-2
    cos = float((got * ref).sum() / (np.linalg.norm(got) * np.linalg.norm(ref)))
    assert cos > 0.999
    # the whole stack against the bf16-emulating oracle (15 layers of bf16 operands and bf16 results, exact accumulation).  The TIGHT
    # statement is per layer (assert_bf16_layer above: never more than one bf16 step, > 97 % of the values identical); through 15 layers
    # those one-step flips are re-amplified by every following contraction (fc6 sums 25088 of them), so end to end the emulation is only
    # somewhat closer than the f32 oracle (measured 5.7e-3 vs 7.6e-3 of the tensor's max) -- bounded here, not claimed equal
    host = ([L.from_jl(t) for t in w[0]], [t.cpu().numpy() for t in w[1]], (L.from_jl(w[2][0]), w[2][1].cpu().numpy()),
            (L.from_jl(w[3][0]), w[3][1].cpu().numpy()))
    with orc.emulate_bf16():
        emu = orc.vgg_forward(host[0], host[1], host[2], host[3], x[:, :, :, :1])
    e1 = rel_max_err(got[:1], emu)
    print("bf16 VGG vs emulating oracle: rel max err %.3e (vs f32 oracle %.3e)" % (e1, rel_max_err(got[:1], ref[:1])))
    assert e1 <= 1e-2


def test_fused_conv1_1_conv1_2_matches_two_launch_path(vgg_setup, monkeypatch):
    # conv64.hip FUSE (conv1_1 computed inside the conv1_2 kernel from the raw uint8 window) against the two-launch path
    # (conv11.hip + conv64.hip) on the same crops: same bf16 operands, conv1_1 summed in a different K order.
    w, img, x, ref = vgg_setup
    rng = np.random.default_rng(99)
    img3 = np.concatenate([img, rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)])
    img3[2, :40] = 255  # saturated / dark bands: exercises ReLU cut-off and the image borders
    img3[2, -30:] = 0
    host = ([L.from_jl(t) for t in w[0]], [t.cpu().numpy() for t in w[1]], (L.from_jl(w[2][0]), w[2][1].cpu().numpy()),
            (L.from_jl(w[3][0]), w[3][1].cpu().numpy()))
    ref3 = orc.vgg_forward(host[0], host[1], host[2], host[3], orc.preprocess_u8(img3[2:3], np.array(L.VGG_MEAN, np.float32)))
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("LRCN_FUSE11", knob)
        ctx = small_ctx(lrcn_amd.LRCN_BF16, max_images=3)
        L.vgg_load(ctx, *w)
        outs[knob] = L.from_jl(L.convnet_u8(ctx, torch.as_tensor(img3).cuda()))
        ctx.close()
        assert rel_max_err(outs[knob][:2], ref) <= 3e-2 and rel_max_err(outs[knob][2:], ref3) <= 3e-2
    assert rel_max_err(outs["1"], outs["0"]) <= 1.5e-2


@pytest.mark.parametrize("gen", ["2", "1"])
@pytest.mark.parametrize("S,N,cap", [(16, 1, 0), (32, 3, 0), (48, 2, 8), (64, 5, 8), (224, 1, 24)])
def test_fused_conv1_launch_vs_emulating_oracle(S, N, cap, gen, monkeypatch):
    # the bf16 stack's first launch by itself (lrcn_conv1_fused): mean subtraction + conv1_1 + ReLU + conv1_2 + ReLU + pool in ONE kernel --
    # gen 2 = conv64f.hip (producer slices inside every wave's half-tap loop, bias in the K padding), gen 1 = conv64.hip FUSE (alternating
    # wave groups) -- value by value against the bf16-EMULATING oracle.  cap = 8 / 24 workgroups: every workgroup walks several tiles
    # (patch-buffer toggling, raw windows three patches ahead, the tail where no tile is left to produce); S = 16: a single tile that is all border.
    monkeypatch.setenv("LRCN_FUSE11_GEN", gen)
    rng = np.random.default_rng(S * 10 + N)
    img = rng.integers(0, 256, size=(N, S, S, 3), dtype=np.uint8)
    img[0, : S // 4] = 255  # a saturated and a dark band: ReLU cut-off at the borders
    img[-1, -S // 4:] = 0
    w11 = (rng.standard_normal((3, 3, 3, 64)) * np.sqrt(2.0 / 27)).astype(np.float32)
    w12 = (rng.standard_normal((3, 3, 64, 64)) * np.sqrt(2.0 / 576)).astype(np.float32)
    b11 = (rng.standard_normal(64) * 20.0).astype(np.float32)  # of the size of the activations: a bias lost or doubled cannot hide
    b12 = (rng.standard_normal(64) * 20.0).astype(np.float32)
    mean = np.array(L.VGG_MEAN, np.float32)
    x = orc.preprocess_u8(img, mean)
    ref = orc.pool2(orc.conv3x3(orc.conv3x3(x, w11, b11, relu=True), w12, b12, relu=True))
    with orc.emulate_bf16():
        a1 = orc.conv3x3(x, w11, b11, relu=True)
        emu = orc.pool2(orc.conv3x3(a1, w12, b12, relu=True))
    ctx = small_ctx(lrcn_amd.LRCN_BF16)
    if cap:
        L.vgg_set_wg_cap(ctx, cap)
    got = L.from_jl(L.conv1_fused(ctx, torch.as_tensor(img).cuda(), mean, L.to_jl(w11), torch.as_tensor(b11).cuda(), L.to_jl(w12),
                                  torch.as_tensor(b12).cuda()))
    ctx.close()
    assert got.shape == ref.shape and (got > 0).any()
    assert rel_max_err(got, ref) <= 2e-2
    # Two chained bf16 layers: where the kernel's f32 sum of conv1_1 lands on the neighbouring bf16 (one step <= 2^-7 relative, ~1e-3 of
    # the values), the conv1_2 sums that read it move by that step times a weight -- little against the tensor, but any number of steps of
    # a sum that cancels to near zero.  So: one output step, plus ONE flipped conv1_1 input at its worst; and nearly every value identical.
    diff = np.abs(got - emu)
    flip = 2.0 ** -7 * float(np.abs(a1).max()) * float(np.abs(w12).max())
    assert (diff <= 2.0 ** -7 * np.abs(emu) + flip).all(), (gen, float(diff.max()), flip)
    assert (diff == 0).mean() > 0.999, float((diff == 0).mean())


# ---------------------------------------------------------------------------------------------- fp8 (BASELINE config 5)
# The absolute term of the e4m3 layers' value-by-value bound, in units of the output scale: four steps of e4m3's grid below 2^-5 (2^-9).
# NOT for the conversion: v_cvt_pk_fp8_f32 is round-to-nearest-even in the subnormal range too (test_gpu_fp8_seams.py, every bf16 pattern).
# It is for the sum: v_mfma_f32_16x16x128_f8f6f4 does not add its 128 products exactly (measured: +448*448 - 448*448 + 126 products of 2^-j
# in ONE K-tile gives 120 * 2^-j for every j = 0 .. 9, the same products without the cancelling pair give 126 * 2^-j), so the accumulator is
# off by up to ~1e-6 of the sum of |products| (10 .. 14 at 1.2e7 in the first case below).  Where acc * escale cancels against a bias of
# thousands of grid steps, that is more than one step of the grid near zero: with 2^-9 here every case below fails, worst 3 steps
# (|d| - 0.126 |emu| = 2.12 steps, on the 512-row tile); above 2^-5 every difference seen is exactly one step.
FP8_ABS_SLACK = 2.0 ** -7


def _fp8_layer(ctx, x, w, b, relu, pool, sa_in=None, sa_out=None, fp32_close=True):
    """One launch of the per-layer e4m3 probe against the same arithmetic carried out on the host; both bounds of
    test_fp8_conv_layer_matches_emulated_arithmetic.  sa_in / sa_out: None = max / 448 (nothing saturates).  Returns (xq, emu / sa_out, y)."""
    Cout = w.shape[3]
    tgt = orc.conv3x3(x, w, b, relu=relu)
    if pool:
        tgt = orc.pool2(tgt)
    sa_in = np.float32(x.max() / 448.0) if sa_in is None else np.float32(sa_in(x))
    sa_out = np.float32(np.abs(tgt).max() / 448.0) if sa_out is None else np.float32(sa_out(tgt))
    y, sw = L.conv3x3_fp8(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), float(sa_in), float(sa_out), relu=relu, pool=pool)
    route = L.debug_route(ctx)
    print("fp8 layer %s Cout=%d relu=%d pool=%d: route %s" % (x.shape, Cout, relu, pool, route))
    assert route.startswith("8p-f8:"), route
    y, sw = L.from_jl(y), sw.cpu().numpy()
    np.testing.assert_allclose(sw, np.abs(w).max(axis=(0, 1, 2)) / np.float32(448.0), rtol=1e-6)
    xq = _e4m3(x * (np.float32(1.0) / sa_in))
    wq = _e4m3(w * (np.float32(1.0) / sw)[None, None, None, :])
    acc = orc.conv3x3(xq, wq, np.zeros(Cout, np.float32), relu=False)
    if pool:
        acc = orc.pool2(acc)
    v = (acc * (sa_in * sw / sa_out)[None, None, :, None] + (b / sa_out)[None, None, :, None]).astype(np.float32)
    q = _e4m3(np.maximum(v, 0.0) if relu else v)
    emu = q * sa_out
    diff = np.abs(y - emu)
    # never more than one e4m3 step (2^-3 relative); near zero (< 0.007 % of the tensor's max) the inexact MFMA sum moves a value that
    # is a cancellation against the bias by up to three steps of 2^-9 (FP8_ABS_SLACK above)
    print("  worst |d| beyond 0.126 |emu|: %.3g subnormal steps; identical %.5f" % (float((diff - 0.126 * np.abs(emu)).max() / (2.0 ** -9 * sa_out)),
                                                                                    float((diff == 0).mean())))
    assert (diff <= 0.126 * np.abs(emu) + FP8_ABS_SLACK * sa_out).all(), float(diff.max())
    assert (diff == 0).mean() > 0.99, float((diff == 0).mean())
    if fp32_close:  # and the quantised layer is close to the fp32 layer: e4m3 keeps 3 mantissa bits per operand and per output
        err = np.linalg.norm(y - tgt) / np.linalg.norm(tgt)
        assert err < 0.06, err
    return xq, q, y


@pytest.mark.parametrize("W,H,Cin,Cout,N", [(16, 16, 128, 128, 1), (16, 16, 256, 256, 2), (12, 20, 128, 512, 3), (28, 28, 512, 512, 1)])
def test_fp8_conv_layer_matches_emulated_arithmetic(W, H, Cin, Cout, N):
    # gemm_8p.hip F8 (v_mfma_f32_16x16x128_f8f6f4, e4m3 staged epilogue): the kernel's result must equal the same
    # arithmetic carried out on the host -- quantise x and w exactly as fp8.hip does, convolve the quantised values with
    # the CPU oracle (fp32), scale / bias / ReLU / pool / e4m3 -- except where fp32 summation order moves a value across
    # an e4m3 rounding boundary (one ulp = 2^-3 relative).  M = N*W*H covers a 256-row tile edge (720) and a full one.
    rng = np.random.default_rng(Cin + Cout + N)
    x = np.abs(rng.standard_normal((W, H, Cin, N))).astype(np.float32)  # post-ReLU-like inputs
    w = (rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.05).astype(np.float32)
    ctx = small_ctx()
    for pool in (False, True):
        _fp8_layer(ctx, x, w, b, True, pool)
    ctx.close()


@pytest.mark.parametrize("case", ["linear", "saturating-input", "saturating-output", "cout-208"])
def test_fp8_conv_layer_linear_saturating_and_column_tail(case):
    """The per-layer e4m3 probe where test_fp8_conv_layer_matches_emulated_arithmetic does not go, same emulation, same two bounds, pool on
    and off: relu = 0 (b ~ 0.5 N(0,1); the emulation has negatives, so the epilogue's lower clamp and signed conversion run);
    sa_in = max / (4 * 448), where the inputs saturate in ref_to_nhwc_fp8_kernel; sa_out = max / (4 * 448), where the outputs saturate
    in the staged epilogue (at least 1 % of the quantised tensor at +-448 in each, and y finite: an unclamped value converts to NaN);
    Cout = 208, a column tail inside the tile.  Tile configs reached (lrcn_debug_route): every case here, Cout = 128 and 208, runs 8p-f8:1
    (256 x 128 tiles); of test_fp8_conv_layer_matches_emulated_arithmetic's cases Cout = 128 runs 8p-f8:1 and Cout = 256, 512 run 8p-f8:0
    (256 x 256); 8p-f8:2 (512 x 128) is reached by test_fp8_conv2_2_on_the_512_row_tile_matches_emulated_arithmetic alone."""
    Cout = 208 if case == "cout-208" else 128
    rng = np.random.default_rng(len(case) + Cout)
    x = np.abs(rng.standard_normal((16, 16, 128, 1))).astype(np.float32)
    w = (rng.standard_normal((3, 3, 128, Cout)) * np.sqrt(2.0 / (9 * 128))).astype(np.float32)
    b = (rng.standard_normal(Cout) * (0.5 if case == "linear" else 0.05)).astype(np.float32)
    ctx = small_ctx()
    for pool in (False, True):
        if case == "linear":
            xq, q, y = _fp8_layer(ctx, x, w, b, False, pool, fp32_close=False)
            assert (q < 0).mean() > 0.1 and (y < 0).any()
        elif case == "saturating-input":
            xq, q, y = _fp8_layer(ctx, x, w, b, True, pool, sa_in=lambda t: t.max() / (4 * 448.0), fp32_close=False)
            assert (np.abs(xq) == 448.0).mean() >= 0.01
        elif case == "saturating-output":
            xq, q, y = _fp8_layer(ctx, x, w, b, True, pool, sa_out=lambda t: t.max() / (4 * 448.0), fp32_close=False)
            assert (np.abs(q) == 448.0).mean() >= 0.01
        else:
            xq, q, y = _fp8_layer(ctx, x, w, b, True, pool)
        assert np.isfinite(y).all()
    ctx.close()


def test_full_vgg_fp8_vs_oracle(vgg_setup):
    # conv2_2 .. conv5_3 in e4m3 (calibrated on the same two images), the rest bf16, against the fp32 CPU oracle.
    # Stated tolerance of the fp8 path: cosine >= 0.99 per image and relative L2 error <= 0.15 on the fc7 features
    # (ten e4m3 layers in sequence; the bf16 path holds 3e-2 of the max).  Not a claim about the reference, which has no
    # reduced-precision path.
    w, img, x, ref = vgg_setup
    ctx = small_ctx(lrcn_amd.LRCN_FP8, max_images=2)
    L.vgg_load(ctx, *w)
    imgs = torch.as_tensor(img).cuda()
    with pytest.raises(lrcn_amd.LrcnError):
        L.convnet_u8(ctx, imgs)  # not calibrated yet
    L.vgg_calibrate(ctx, imgs)
    got = L.from_jl(L.convnet_u8(ctx, imgs))
    assert np.isfinite(got).all()
    for n in range(2):
        cos = float((got[n] * ref[n]).sum() / (np.linalg.norm(got[n]) * np.linalg.norm(ref[n])))
        rel = float(np.linalg.norm(got[n] - ref[n]) / np.linalg.norm(ref[n]))
        print("fp8 vgg image %d: cosine %.5f rel L2 %.4f" % (n, cos, rel))
        assert cos >= 0.99 and rel <= 0.15, (cos, rel)
    got1 = L.from_jl(L.convnet_u8(ctx, imgs[1:2]))
    np.testing.assert_allclose(got1[0], got[1], rtol=0, atol=1e-5 * np.abs(ref).max())
    ctx.close()


@pytest.mark.parametrize("conv64", ["1", "0"], ids=["direct", "cast"])
def test_fp8_forward_of_images_outside_the_calibrated_range_saturates_and_stays_finite(vgg_setup, conv64, monkeypatch):
    """On both conv2_1 -> conv2_2 routes (LRCN_CONV64=0: the cast).  Calibrated on low-contrast crops (img // 8 + 112) with margin 1, then run on the full-contrast ones: activations beyond 448 sa meet the
    clamp in front of every e4m3 conversion (conv64.hip's epilogue, the staged epilogue of gemm_8p.hip; fp8.hip's cast on the other route) --
    an unclamped one converts to the NaN byte and poisons the features.  Every feature is finite, the features differ from those of a
    context calibrated on the images themselves (the saturation is real), a second forward gives the same bits.  No accuracy is claimed for
    a saturated forward."""
    w, img, x, ref = vgg_setup
    imgs = torch.as_tensor(img).cuda()
    monkeypatch.setenv("LRCN_CONV64", conv64)
    ctx = small_ctx(lrcn_amd.LRCN_FP8, max_images=2)
    L.vgg_load(ctx, *w)
    L.vgg_calibrate(ctx, torch.as_tensor(img // 8 + 112).cuda(), margin=1.0)
    narrow = L.debug_fp8_scales(ctx)
    got = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    assert ("conv64" in L.debug_route(ctx, 1)) == (conv64 == "1"), L.debug_route(ctx, 1)
    again = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    L.vgg_calibrate(ctx, imgs, margin=1.0)
    wide = L.debug_fp8_scales(ctx)
    own = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    ctx.close()
    assert (narrow[2:] < wide[2:]).all(), (narrow, wide)
    assert np.isfinite(got).all() and (got != 0).any()
    np.testing.assert_array_equal(again, got)
    print("saturated forward vs own calibration: rel max difference %.3f" % rel_max_err(got, own))
    assert np.isfinite(own).all() and (got != own).any()


def test_full_vgg_fp8_cast_route_vs_oracle(vgg_setup, monkeypatch):
    """LRCN_CONV64=0 on an fp8 context: conv2_1 runs on a kernel without the e4m3 epilogue, so cast_bf16_fp8_kernel stands in front of
    conv2_2 (and conv11.hip in front of the stack) -- the second of the two conv2_1 -> conv2_2 routes.  No conv64 kernel in the routes; the
    fp8 path's stated bounds against the fp32 oracle, as test_full_vgg_fp8_vs_oracle.  Not compared bitwise with the direct route: that one
    quantises the f32 sum, this one its bf16 rounding.
    Calibrated on the images it runs, nothing saturates here: a cast_bf16_fp8_kernel without its clamp passes this test and fails
    test_gpu_fp8_seams.py's exhaustive cast test."""
    w, img, x, ref = vgg_setup
    imgs = torch.as_tensor(img).cuda()
    monkeypatch.setenv("LRCN_CONV64", "0")
    ctx = small_ctx(lrcn_amd.LRCN_FP8, max_images=2)
    L.vgg_load(ctx, *w)
    L.vgg_calibrate(ctx, imgs)
    got = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    routes = L.debug_route(ctx, 1).split(",")
    ctx.close()
    assert routes[0] == "conv11" and len(routes) == 15 and not any("conv64" in r for r in routes), routes
    assert all(r.startswith("8p-f8:") for r in routes[3:13]), routes
    assert np.isfinite(got).all()
    for n in range(2):
        cos = float((got[n] * ref[n]).sum() / (np.linalg.norm(got[n]) * np.linalg.norm(ref[n])))
        rel = float(np.linalg.norm(got[n] - ref[n]) / np.linalg.norm(ref[n]))
        print("fp8 vgg, cast route, image %d: cosine %.5f rel L2 %.4f" % (n, cos, rel))
        assert cos >= 0.99 and rel <= 0.15, (cos, rel)


def test_capped_persistent_conv_grids_are_bit_identical(vgg_setup):
    # lrcn_vgg_set_wg_cap: the convolution kernels walk several tiles per workgroup (cap 8: up to 49 tiles each here;
    # cap 224: what the data-parallel step uses) -- same tiles, same arithmetic, so the features must not change at all.
    w, img, x, ref = vgg_setup
    imgs = torch.as_tensor(np.concatenate([img, img[::-1]])).cuda()
    for dt in (lrcn_amd.LRCN_BF16, lrcn_amd.LRCN_FP8):
        ctx = small_ctx(dt, max_images=4)
        L.vgg_load(ctx, *w)
        if dt == lrcn_amd.LRCN_FP8:
            L.vgg_calibrate(ctx, imgs)
        base = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
        for cap in (8, 224):
            L.vgg_set_wg_cap(ctx, cap)
            np.testing.assert_array_equal(L.from_jl(L.convnet_u8(ctx, imgs)), base)
        with pytest.raises(lrcn_amd.LrcnError):
            L.vgg_set_wg_cap(ctx, 3)
        ctx.close()


def test_pulled_tiles_under_a_cap_are_bit_identical(vgg_setup, monkeypatch):
    """LRCN_DYN_TILES=1 under a cap: the workgroups of gemm8p_kernel PULL their tiles from eight per-XCD queues (atomic claims, the claimed
    id handed to the other waves through a per-workgroup global slot) instead of walking static shares.  An opt-in knob, measured and
    left off -- and until now run by no test.  Which workgroup computes a tile does not enter its arithmetic: for bf16 and fp8, 4 images,
    caps 8 and 224, the features are the bits of the uncapped forward of the same context, on the same routes as with the knob unset."""
    w, img, x, ref = vgg_setup
    imgs = torch.as_tensor(np.concatenate([img, img[::-1]])).cuda()
    for dt in (lrcn_amd.LRCN_BF16, lrcn_amd.LRCN_FP8):
        ctx = small_ctx(dt, max_images=4)
        L.vgg_load(ctx, *w)
        if dt == lrcn_amd.LRCN_FP8:
            L.vgg_calibrate(ctx, imgs)
        base = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
        assert np.isfinite(base).all() and (base != 0).any()
        for cap in (8, 224):
            L.vgg_set_wg_cap(ctx, cap)
            walked = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
            routes = L.debug_route(ctx, 1)
            monkeypatch.setenv("LRCN_DYN_TILES", "1")
            pulled = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
            pulled_routes = L.debug_route(ctx, 1)
            monkeypatch.delenv("LRCN_DYN_TILES")
            assert pulled_routes == routes and any(r.startswith("8p") for r in routes.split(",")), (cap, routes, pulled_routes)
            np.testing.assert_array_equal(walked, base)
            np.testing.assert_array_equal(pulled, base)
        ctx.close()


def test_config2_end_to_end_fp32_images_to_loss(vgg_setup):
    # BASELINE configs[1] composed end to end in fp32 on the parity scale: uint8 crops -> VGG-16 -> fc7 (exact-fp32 MFMA)
    # -> LSTM-512 loss and gradients, against the CPU oracle run on the same crops (features and loss from the oracle's
    # own VGG forward).  Two images; the full-size shapes are covered by test_gpu_fullsize.py / test_config1_shape_*.
    w, img, x, ref = vgg_setup
    E = H = 512
    V, T, B = 2540, 11, 2
    rng = np.random.default_rng(12)
    m = orc.init_weights(E, H, H, V, seed=42)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    fn = (ref / ref.sum(axis=1, keepdims=True)).astype(np.float32)  # the reference trains on sum-normalised features
    ref_loss, ref_g = orc.loss(m, fn, tokens, want_grad=True)
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, vgg_dtype=lrcn_amd.LRCN_F32, max_images=B)
    L.vgg_load(ctx, *w)
    feats = L.from_jl(L.convnet_u8(ctx, torch.as_tensor(img).cuda()))
    feats = (feats / feats.sum(axis=1, keepdims=True)).astype(np.float32)
    grads, val = L.lossgradient(ctx, L.model_from_arrays(m.p), L.to_jl(feats), tokens)
    assert abs(val - ref_loss) <= 1e-4 * abs(ref_loss), (val, ref_loss)
    for n, g in zip(orc.PARAM_NAMES, grads):
        a, b = L.from_jl(g).ravel().astype(np.float64), ref_g.p[n].ravel().astype(np.float64)
        assert np.linalg.norm(a - b) <= 2e-3 * np.linalg.norm(b) + 1e-9, n
    ctx.close()


# ------------------------------------------------------- conv1_1 by itself and the float-input forward (include/lrcn_conv_debug.h)
CONV11_MEAN = (135.68, 116.779, 97.939)   # the three channels differ by more than 10: a swapped channel or mean moves every pixel


def _conv11_case(S, N):
    rng = np.random.default_rng(S * 10 + N)
    img = rng.integers(0, 256, size=(N, S, S, 3), dtype=np.uint8)
    img[0, : S // 4] = 255  # a saturated and a dark band: ReLU cut-off at the borders
    img[-1, -S // 4:] = 0
    w11 = (rng.standard_normal((3, 3, 3, 64)) * np.sqrt(2.0 / 27)).astype(np.float32)
    b11 = (rng.standard_normal(64) * 20.0).astype(np.float32)  # of the size of the activations: a bias lost or doubled cannot hide
    return img, w11, b11


@pytest.mark.parametrize("dtype", [lrcn_amd.LRCN_BF16, lrcn_amd.LRCN_FP8], ids=["bf16", "fp8"])
@pytest.mark.parametrize("S,N", [(6, 1), (16, 1), (18, 3), (224, 1)])
def test_conv11_launch_vs_emulating_oracle(S, N, dtype):
    """conv11.hip by itself (lrcn_debug_conv11), from uint8 crops (conv11_kernel<true>) and from the preprocessed float tensor
    (conv11_kernel<false>: what lrcn_vgg_forward runs on a bf16 or fp8 context, and the average-image path outside the fused first launch),
    value by value against the bf16-emulating oracle.  36 rows: one partial block, every pixel on or beside the border; 256: exactly one
    block; 972: three blocks and a 204-row tail, image seams inside blocks (rows 324 and 648); 50176: the product geometry.  Both sources
    are the same bf16 operands in the same kernel: bit for bit.  (An fp8 context runs conv1_1 in bf16 like a bf16 one: same bounds.)
    A local build (not kept) whose conv11_kernel<false> read f[y + S * x] for f[x + S * y] failed every case at the float source's
    assert_bf16_layer (worst |d| 492 .. 568 at max|ref| 440 .. 568) and both whole-stack tests at their bitwise comparison."""
    img, w11, b11 = _conv11_case(S, N)
    mean = np.array(CONV11_MEAN, np.float32)
    x = orc.preprocess_u8(img, mean)
    with orc.emulate_bf16():
        emu = orc.conv3x3(x, w11, b11, relu=True)
    ctx = small_ctx(dtype)
    w, b = L.to_jl(w11), torch.as_tensor(b11).cuda()
    got8 = L.from_jl(L.debug_conv11(ctx, torch.as_tensor(img).cuda(), w, b, mean=CONV11_MEAN))
    gotf = L.from_jl(L.debug_conv11(ctx, L.to_jl(x), w, b))
    ctx.close()
    assert got8.shape == emu.shape == (S, S, 64, N) and (emu > 0).any() and (emu == 0).any()
    assert_bf16_layer(got8, emu, "uint8 source S=%d N=%d" % (S, N))
    assert_bf16_layer(gotf, emu, "float source S=%d N=%d" % (S, N))
    np.testing.assert_array_equal(gotf, got8)


def test_conv11_launch_refuses_bad_arguments_before_any_launch():
    img, w11, b11 = _conv11_case(6, 1)
    w, b = L.to_jl(w11), torch.as_tensor(b11).cuda()
    lib = lrcn_amd._lib.lib()
    mean = (ctypes.c_float * 3)(*CONV11_MEAN)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ctx = small_ctx(lrcn_amd.LRCN_BF16)
    y = L.jl_empty(8, 8, 64, 1)
    y.fill_(123.0)
    u8 = torch.as_tensor(np.zeros((1, 8, 8, 3), np.uint8)).cuda()
    torch.cuda.synchronize()
    for args in ((p(u8), 1, 1, 7, mean, p(w), p(b), p(y)),      # odd S
                 (p(u8), 1, 1, 0, mean, p(w), p(b), p(y)),      # S < 2
                 (p(u8), 1, 0, 8, mean, p(w), p(b), p(y)),      # N < 1
                 (p(u8), 1, 1, 8, None, p(w), p(b), p(y)),      # a uint8 source needs the means
                 (None, 0, 1, 8, None, p(w), p(b), p(y)), (p(u8), 1, 1, 8, mean, None, p(b), p(y)),
                 (p(u8), 1, 1, 8, mean, p(w), None, p(y)), (p(u8), 1, 1, 8, mean, p(w), p(b), None)):
        assert lib.lrcn_debug_conv11(ctx._h, *args) == -1, args[1:4]
    assert lib.lrcn_debug_conv11(None, p(u8), 1, 1, 8, mean, p(w), p(b), p(y)) == -1
    ctx.close()
    f32 = small_ctx(lrcn_amd.LRCN_F32)   # the f32 stack has no conv11.hip: its conv1_1 is an im2col GEMM
    assert lib.lrcn_debug_conv11(f32._h, p(u8), 1, 1, 8, mean, p(w), p(b), p(y)) == -1
    f32.close()
    torch.cuda.synchronize()
    assert bool((y == 123.0).all())


def test_float_input_forward_bf16(vgg_setup, monkeypatch):
    """lrcn_vgg_forward (the entry INTEGRATION.md maps to the reference's convnet) on a bf16 context: conv11_kernel<false> in front of the
    stack.  Two launches (LRCN_FUSE11=0): the float tensor that lrcn_preprocess_u8 makes of the crops gives the uint8 entry's bits, with the
    channel means and with an average image (where the uint8 entry itself goes through the float route).  Default knobs: against the fp32
    oracle and against the fused uint8 entry with this file's constants."""
    w, img, x, ref = vgg_setup
    imgs = torch.as_tensor(img).cuda()
    avg = (np.random.default_rng(8).standard_normal((224, 224, 3)) * 20.0 + np.array(L.VGG_MEAN)).astype(np.float32)
    monkeypatch.setenv("LRCN_FUSE11", "0")
    ctx = small_ctx(lrcn_amd.LRCN_BF16, max_images=2)
    L.vgg_load(ctx, *w)
    got8 = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    assert L.debug_route(ctx, 1).split(",")[0] == "conv11"
    gotf = L.from_jl(L.convnet(ctx, L.read_image_data_u8(ctx, imgs))).copy()
    assert L.debug_route(ctx, 1).split(",")[0] == "conv11"
    np.testing.assert_array_equal(gotf, got8)
    assert rel_max_err(got8, ref) <= 3e-2
    L.set_average_image(ctx, avg)
    a8 = L.from_jl(L.convnet_u8(ctx, imgs, mean=None)).copy()
    af = L.from_jl(L.convnet(ctx, L.read_image_data_u8(ctx, imgs, mean=None))).copy()
    np.testing.assert_array_equal(af, a8)
    assert np.abs(a8 - got8).max() > 0   # the average image is not the channel means
    ctx.close()
    monkeypatch.delenv("LRCN_FUSE11")
    ctx = small_ctx(lrcn_amd.LRCN_BF16, max_images=2)
    L.vgg_load(ctx, *w)
    fused8 = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    assert L.debug_route(ctx, 1).split(",")[0] == "conv64-fused11"
    gotf = L.from_jl(L.convnet(ctx, L.to_jl(x))).copy()
    assert L.debug_route(ctx, 1).split(",")[0] == "conv11"
    ctx.close()
    assert gotf.shape == (2, 4096) and (gotf < 0).any()
    assert rel_max_err(gotf, ref) <= 3e-2
    assert float((gotf * ref).sum() / (np.linalg.norm(gotf) * np.linalg.norm(ref))) > 0.999
    assert rel_max_err(gotf, fused8) <= 1.5e-2


def test_float_input_forward_fp8(vgg_setup, monkeypatch):
    # the same bitwise statement on a calibrated fp8 context: conv1_1 .. conv2_1 are bf16 there, conv11_kernel<false> in front
    w, img, x, ref = vgg_setup
    imgs = torch.as_tensor(img).cuda()
    monkeypatch.setenv("LRCN_FUSE11", "0")
    ctx = small_ctx(lrcn_amd.LRCN_FP8, max_images=2)
    L.vgg_load(ctx, *w)
    L.vgg_calibrate(ctx, imgs)
    got8 = L.from_jl(L.convnet_u8(ctx, imgs)).copy()
    gotf = L.from_jl(L.convnet(ctx, L.read_image_data_u8(ctx, imgs))).copy()
    assert L.debug_route(ctx, 1).split(",")[0] == "conv11"
    np.testing.assert_array_equal(gotf, got8)
    assert np.isfinite(got8).all() and (got8 != 0).any()
    # and with an average image, where the uint8 entry itself preprocesses into a float tensor first
    L.set_average_image(ctx, (np.random.default_rng(8).standard_normal((224, 224, 3)) * 20.0 + np.array(L.VGG_MEAN)).astype(np.float32))
    a8 = L.from_jl(L.convnet_u8(ctx, imgs, mean=None)).copy()
    af = L.from_jl(L.convnet(ctx, L.read_image_data_u8(ctx, imgs, mean=None))).copy()
    ctx.close()
    np.testing.assert_array_equal(af, a8)
    assert np.isfinite(a8).all() and np.abs(a8 - got8).max() > 0


def test_fp8_conv2_2_on_the_512_row_tile_matches_emulated_arithmetic():
    """The e4m3 convolution on the 512 x 128 tile (route 8p-f8:2): conv2_2's geometry from 17 images, the smallest batch with >= 400 row
    tiles of 512 (416.5: the last tile is half full).  test_fp8_conv_layer_matches_emulated_arithmetic stops at 784 rows (configs 0 and 1);
    here images 0 and 16 -- the first tiles and the half-full last one -- go through the same per-image host emulation and the same two
    bounds."""
    W = H = 112
    Cin = Cout = 128
    N = 17
    rng = np.random.default_rng(Cin + Cout + N)
    x = np.abs(rng.standard_normal((W, H, Cin, N), dtype=np.float32))  # post-ReLU-like inputs
    w = (rng.standard_normal((3, 3, Cin, Cout)) * np.sqrt(2.0 / (9 * Cin))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.05).astype(np.float32)
    sample = [0, N - 1]
    xs = np.ascontiguousarray(x[..., sample])
    tgt = orc.pool2(orc.conv3x3(xs, w, b, relu=True))
    sa_in = np.float32(x.max() / 448.0)
    sa_out = np.float32(1.25 * tgt.max() / 448.0)   # the two sampled images' range with a margin for the fifteen others
    ctx = small_ctx()
    y, sw = L.conv3x3_fp8(ctx, L.to_jl(x), L.to_jl(w), torch.as_tensor(b).cuda(), float(sa_in), float(sa_out), relu=True, pool=True)
    assert L.debug_route(ctx) == "8p-f8:2"
    y, sw = L.from_jl(y)[..., sample], sw.cpu().numpy()
    ctx.close()
    np.testing.assert_allclose(sw, np.abs(w).max(axis=(0, 1, 2)) / np.float32(448.0), rtol=1e-6)
    xq = _e4m3(xs * (np.float32(1.0) / sa_in))
    wq = _e4m3(w * (np.float32(1.0) / sw)[None, None, None, :])
    acc = orc.pool2(orc.conv3x3(xq, wq, np.zeros(Cout, np.float32), relu=False))
    v = np.maximum(acc * (sa_in * sw / sa_out)[None, None, :, None] + (b / sa_out)[None, None, :, None], 0.0).astype(np.float32)
    emu = _e4m3(v) * sa_out
    assert y.shape == emu.shape == (56, 56, 128, 2) and (emu > 0).mean() > 0.5
    for k, n in enumerate(sample):
        diff = np.abs(y[..., k] - emu[..., k])
        print("  image %d: worst |d| beyond 0.126 |emu|: %.3g subnormal steps" % (n, float((diff - 0.126 * np.abs(emu[..., k])).max() / (2.0 ** -9 * sa_out))))
        assert (diff <= 0.126 * np.abs(emu[..., k]) + FP8_ABS_SLACK * sa_out).all(), (n, float(diff.max()))
        assert (diff == 0).mean() > 0.99, (n, float((diff == 0).mean()))
