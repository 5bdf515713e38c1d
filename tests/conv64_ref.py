"""Exact host references and the case tables of the first-layer halo-patch kernels (tests only; no GPU, nothing of the code under test).

Three kernels run in front of the GEMM engines' convolution mode: conv64.hip's conv64_kernel<POOL, FUSE> (conv1_2 / conv2_1: a three-patch
ring walked persistently under a workgroup cap; FUSE: conv1_1 produced inside it), conv64f.hip (the default first launch: conv1_1 + conv1_2
+ pool, a two-patch toggle, four raw windows fetched three patches ahead, conv1_1's bias cut into three bf16 pieces in the K padding) and
conv11.hip (conv1_1 alone).  Every case here is in an integer regime in which the value each kernel must write is decided with no tolerance.

PLAIN -- conv64_kernel<POOL, false> through lrcn_debug_conv64 (include/lrcn_conv_debug.h).  conv_gemm_ref's Case / Problem with Cin = 64 and
route "conv64": the same integer regime and input conditions (check_int_conditions), the same layout (margins of 2^15 around x, so a halo
that is not taken from the zero page reads 2^15; a guard row and a lead-in of C_SENTINEL around y; y's interior starts as C_STALE).  The
launcher's grid rule (launch_conv64) is restated in grid(): G = max(1, (cap >= 8 ? cap : 256) / (Cout / 64)) workgroups per 64-channel
chunk, clamped to the tile count; workgroup b walks tiles b, b + G, ...  walks() gives the walk lengths each table row is there for.

FUSED -- lrcn_conv1_fused (cap through lrcn_vgg_set_wg_cap), LRCN_FUSE11_GEN=2 (conv64f.hip) and =1 (conv64_kernel<true, true>).  float64
throughout, then cast:
    x   = pixel - mean             integer means that all differ (104, 117, 124): |x| <= 255 is exact in bf16
    a1  = bf16(relu(conv(x, w11) + b11))        ONE torch cast f64 -> f32 (exact) -> bf16
    out = bf16(pool2(relu(conv(a1, w12) + b12)))
w11 are integers in [-2, 2].  b11 is a multiple of 2^-8 in every channel; 36 channels lie in +-[512, 600] with an odd numerator chosen so
that the value needs all THREE bf16 pieces hi + mid + lo (checked with the pieces computed here: below 512 a multiple of 2^-8 always fits two
round-to-nearest pieces, so "17 significant bits" alone does not reach the third), 20 in [64, 256), 8 are negative.  Conditions on the
INPUTS, asserted for every case (they are not tolerances):
  * conv1_1: every term and b11 are multiples of 2^-8 and 27 max|x| max|w11| + max|b11| < 2^15: any partial sum in any order fits a 23-bit
    window and is exact in an f32 accumulator; so is each bias piece times 1.0.
  * conv1_2: 576 max(a1) max|w12| + max|b12| < 2^24, AND, because a1 is not an integer -- its values below 128 keep b11's fractional bits
    through the bf16 rounding, so every term is a multiple of 2^-8 only -- for every output the larger of the sum of its positive and of its
    negative terms, plus |b12|, stays below 2^16: then every partial sum of any subset in any order is a multiple of 2^-8 below 2^16, a
    24-bit window.  The first bound alone does not give exactness.  That is why w12 is sparse: -1 / 0 / +1 with probabilities
    0.09 / 0.82 / 0.09 (every input channel and tap still feeds ~11 of the 64 output channels).  b12 are integers.
  * both signs occur before each ReLU and each ReLU cuts at least 5 %; at least 25 % of a1 is moved by its bf16 rounding; at least half
    of the written outputs exceed 2^8 and some exceed 2^11; at least 32 channels of b11 have three non-zero pieces.

CONV11 -- lrcn_debug_conv11 against the first stage (a1) of the same reference, from the uint8 crops with the integer means and from the
float tensor that holds the same integers.

Layouts: everything here is "internal" NHWC, [n][r][q][c] with q = the reference tensors' dimension 1 (the image row of a crop) and r =
their dimension 2 (the image column), weights [co][kh * 3 + kw][c] with kw along q -- conv_gemm_ref.conv_taps's convention.  to_ref_x /
to_ref_w / from_ref_y convert to and from the reference layouts ((W, H, C, N) and (3, 3, Cin, Cout), first index fastest) that the ABI takes.
"""
import functools
import zlib

import numpy as np
import torch

from conv_gemm_ref import Case, Problem, conv_taps, pool2  # noqa: F401

MEAN = (104.0, 117.0, 124.0)


# ------------------------------------------------------------------------------------------------------------------------------- plain
def _plain_table():
    c = []

    def row(W, H, N, Cout, cap, r=False):
        """Every row runs with the maximum off and on; a row marked r also with a ReLU and a bias."""
        for relu in ((False, True) if r else (False,)):
            for pool in (False, True):
                c.append(Case("conv64", W, H, N, 64, Cout, relu=relu, pool=pool, wg_cap=cap))

    row(16, 16, 1, 64, 0)              # 1 tile on 1: one all-border tile; tile_at(1) = -1 in the prologue
    row(48, 32, 3, 64, 8, r=True)      # 18 on 8: walks of 3 and 2; W != H; image seams inside a walk
    row(32, 32, 5, 128, 8, r=True)     # 20 on 4 x 2 chunks: walks of 5, the ring wraps (j = 3, 4)
    row(48, 48, 3, 128, 8, r=True)     # 27 on 4: walks 7, 7, 7, 6; the centre tile has no border
    row(16, 32, 2, 576, 8)             # 4 on 1 x 9 chunks: cap / chunks = 0 -> 1, one workgroup walks everything
    row(16, 16, 87, 192, 0, r=True)    # 87 on 85 x 3: uncapped, two workgroups walk 2
    row(16, 16, 258, 64, 0)            # 258 on 256: the uncapped grid's own limit
    return c


PLAIN_CASES = _plain_table()
# (W, H, N, Cout, cap) -> (tiles, G, the walk lengths the row is in the table for)
PLAIN_WALKS = {
    (16, 16, 1, 64, 0): (1, 1, {1}),
    (48, 32, 3, 64, 8): (18, 8, {3, 2}),
    (32, 32, 5, 128, 8): (20, 4, {5}),
    (48, 48, 3, 128, 8): (27, 4, {7, 6}),
    (16, 32, 2, 576, 8): (4, 1, {4}),
    (16, 16, 87, 192, 0): (87, 85, {2, 1}),
    (16, 16, 258, 64, 0): (258, 256, {2, 1}),
}


def grid(tiles, chunks, cap):
    """launch_conv64's rule (chunks = Cout / 64; the fused launches have chunks = 1): workgroups per chunk."""
    return min(max(1, (cap if cap >= 8 else 256) // chunks), tiles)


def walks(tiles, G):
    """Tiles walked by workgroup b = 0 .. G - 1 (tiles b, b + G, ...)."""
    return [(tiles - b + G - 1) // G for b in range(G)]


# ------------------------------------------------------------------------------------------------------------------------------- fused
FUSED_CASES = [(16, 1, 0), (32, 3, 0), (16, 9, 8), (16, 19, 8), (48, 2, 8), (48, 5, 8), (16, 258, 0), (224, 1, 24)]   # (S, N, cap)
# (S, N, cap) -> (tiles, G, walk lengths)
FUSED_WALKS = {
    (16, 1, 0): (1, 1, {1}),
    (32, 3, 0): (12, 12, {1}),
    (16, 9, 8): (9, 8, {2, 1}),       # raw issues (three patches ahead) of tiles that do not exist
    (16, 19, 8): (19, 8, {3, 2}),
    (48, 2, 8): (18, 8, {3, 2}),      # an interior tile
    (48, 5, 8): (45, 8, {6, 5}),      # the four raw buffers wrap, the patch buffers toggle
    (16, 258, 0): (258, 256, {2, 1}),
    (224, 1, 24): (196, 24, {9, 8}),  # product geometry
}
CONV11_CASES = [(6, 1), (16, 1), (18, 3), (224, 1)]   # (S, N): test_gpu_vgg_parity.py's geometries of lrcn_debug_conv11


def bf16_pieces(b):
    """A float32 tensor cut as k_repack_conv11_w_fused cuts conv1_1's bias: hi = bf16(b), mid = bf16(b - hi), lo = bf16(b - hi - mid), each
    round-to-nearest-even, as float32."""
    b = b.float()
    hi = b.bfloat16().float()
    mid = (b - hi).bfloat16().float()
    lo = (b - hi - mid).bfloat16().float()
    return hi, mid, lo


def make_b11(rng):
    """conv1_1's bias: multiples of 2^-8.  Channels 0..35 (shuffled afterwards): +-[512, 600) with a remainder that needs the third piece;
    20 channels in [64, 256); 8 negative in [-400, -64]."""
    b = np.zeros(64)
    k = 0
    while k < 36:
        v = float(rng.integers(512, 600)) + float(2 * rng.integers(0, 128) + 1) / 256.0
        if all(float(p) != 0.0 for p in bf16_pieces(torch.tensor([v]))):
            b[k] = v
            k += 1
    b[36:56] = rng.integers(64, 256, size=20) + rng.integers(0, 256, size=20) / 256.0
    b[56:64] = -(rng.integers(64, 400, size=8) + rng.integers(0, 256, size=8) / 256.0)
    b[34:36] = -b[34:36]   # two of the three-piece values negative: ReLU cuts nearly all of those channels
    rng.shuffle(b)
    return torch.from_numpy(b)


class Stage1:
    """The crops, conv1_1's operands and a1 = bf16(relu(conv(x, w11) + b11)) of S x S x N crops, with the conditions on them asserted."""

    def __init__(self, S, N):
        self.S, self.N = S, N
        rng = np.random.default_rng(zlib.crc32(("stage1 %d %d" % (S, N)).encode()))
        img = rng.integers(0, 256, size=(N, S, S, 3), dtype=np.uint8)
        img[0, : max(S // 8, 1)] = 255      # a saturated and a dark band at two image borders
        img[-1, :, -max(S // 8, 1):] = 0
        self.img = torch.from_numpy(img)                                     # [n][row = q][column = r][c]
        self.mean = torch.tensor(MEAN, dtype=torch.float64)
        self.x = self.img.permute(0, 2, 1, 3).double() - self.mean          # internal [n][r][q][c]
        self.w11 = torch.from_numpy(rng.integers(-2, 3, size=(64, 9, 3)).astype(np.float64))
        self.b11 = make_b11(rng)
        self.pre1 = conv_taps(self.x, self.w11) + self.b11                   # [n][r][q][64]
        exact = self.pre1.clamp_min(0.0)
        self.a1 = exact.float().bfloat16()                                   # f64 -> f32 is exact (23-bit window), then ONE rounding
        self.moved = float((self.a1.double() != exact).double().mean())
        self.check()

    def check(self):
        tag = ("stage1", self.S, self.N)
        assert len(set(MEAN)) == 3 and all(m == int(m) for m in MEAN)
        assert float(self.x.abs().max()) <= 255 and torch.equal(self.x, self.x.float().bfloat16().double()), tag
        b256 = self.b11 * 256.0
        assert torch.equal(b256, b256.round()) and torch.equal(self.b11, self.b11.float().double()), tag   # multiples of 2^-8, exact in f32
        head = 27 * float(self.x.abs().max()) * float(self.w11.abs().max()) + float(self.b11.abs().max())
        assert head < 2 ** 15, (tag, head)
        hi, mid, lo = bf16_pieces(self.b11)
        assert torch.equal((hi.double() + mid.double() + lo.double()), self.b11), tag
        three = (hi != 0) & (mid != 0) & (lo != 0)
        assert int(three.sum()) >= 32, (tag, int(three.sum()))
        assert int((self.b11 > 0).sum()) >= 48 and int((self.b11 < 0).sum()) >= 4, tag
        cut = float((self.pre1 < 0).double().mean())
        assert (self.pre1 > 0).any() and cut >= 0.05, (tag, cut)
        assert self.moved >= 0.25, (tag, self.moved)


@functools.lru_cache(maxsize=2)
def stage1(S, N):
    return Stage1(S, N)


class Fused:
    """Stage1 plus conv1_2's operands and out = bf16(pool2(relu(conv(a1, w12) + b12))), internal layout [n][r / 2][q / 2][64]."""

    def __init__(self, S, N):
        self.S, self.N = S, N
        self.s1 = s1 = stage1(S, N)
        rng = np.random.default_rng(zlib.crc32(("fused %d %d" % (S, N)).encode()))
        self.w12 = torch.from_numpy(rng.choice(np.array([-1.0, 0.0, 1.0]), p=[0.09, 0.82, 0.09], size=(64, 9, 64)))
        self.b12 = torch.from_numpy((16 * rng.integers(-64, 65, size=64)).astype(np.float64))
        a1 = s1.a1.double()
        self.pre2 = conv_taps(a1, self.w12) + self.b12
        mag = conv_taps(a1, self.w12.abs())                                   # sum of |terms|
        conv = self.pre2 - self.b12
        self.side = float((torch.maximum(mag + conv, mag - conv) / 2 + self.b12.abs()).max())   # larger one-signed sum + |b12|
        self.out64 = pool2(self.pre2.clamp_min(0.0))
        self.expected = self.out64.float().bfloat16()
        self.check()

    def check(self):
        tag = ("fused", self.S, self.N)
        a1 = self.s1.a1.double()
        assert torch.equal(a1 * 256.0, (a1 * 256.0).round()), tag            # a1 keeps multiples of 2^-8
        assert torch.equal(self.b12, self.b12.round()) and torch.equal(self.w12, self.w12.round()), tag
        self.head2 = 576 * float(a1.max()) * float(self.w12.abs().max()) + float(self.b12.abs().max())
        assert self.head2 < 2 ** 24, (tag, self.head2)
        assert self.side < 2 ** 16, (tag, self.side)                          # any partial sum: a multiple of 2^-8 below 2^16
        self.cut2 = float((self.pre2 < 0).double().mean())
        assert (self.pre2 > 0).any() and self.cut2 >= 0.05, (tag, self.cut2)
        out = self.out64
        self.big = float((out > 2 ** 8).double().mean())
        assert self.big >= 0.5 and (out > 2 ** 11).any(), (tag, self.big)
        assert torch.equal(self.out64.float().double(), self.out64), tag     # f64 -> f32 exact


@functools.lru_cache(maxsize=1)
def fused(S, N):
    return Fused(S, N)


# ------------------------------------------------------------------------------------------------------------------------------- layouts
def to_ref_x(t):
    """internal [n][r][q][c] -> reference (W, H, C, N) indices [q][r][c][n] (a torch view; L.to_jl makes it first-index-fastest)."""
    return t.permute(2, 1, 3, 0)


def to_ref_w(w):
    """[co][kh * 3 + kw][c] -> reference (3, 3, Cin, Cout) indices [kw][kh][c][co]."""
    return w.reshape(w.shape[0], 3, 3, w.shape[2]).permute(2, 1, 3, 0)


def from_ref_y(y):
    """numpy (W, H, C, N) [q][r][co][n] -> torch internal [n][r][q][co]."""
    return torch.from_numpy(np.ascontiguousarray(np.transpose(y, (3, 1, 0, 2))))


def describe(got, want, limit=4):
    """Where two [n][r][q][c] tensors differ (a NaN never equals): the count and the first few (image, y, x, channel) with got / expected."""
    g, w = got.double(), want.double()
    bad = ~(g == w)
    idx = bad.nonzero()
    first = ["(%d, %d, %d, %d): got %r, expected %r" % (*i.tolist(), float(g[tuple(i)]), float(w[tuple(i)])) for i in idx[:limit]]
    where = ["images %s" % idx[:, 0].unique()[:12].tolist(), "rows y %s" % idx[:, 1].unique()[:24].tolist(),
             "columns x %s" % idx[:, 2].unique()[:24].tolist(), "%d distinct channels" % idx[:, 3].unique().numel()]
    return "%d of %d elements differ; %s; first (image, y, x, channel): %s" % (idx.shape[0], bad.numel(), "; ".join(where), "; ".join(first))
