"""Exact host references and the case table of the GEMM engines' convolution mode (tests only; no GPU, nothing of the code under test).

y[n][r][q][co] = sum_{kh, kw, c} x[n][r + kh - 1][q + kw - 1][c] w[co][kh * 3 + kw][c] (+ bias[co]) (ReLU) (2x2 maximum): the CONV3 operand
mode of csrc/gemm.h with its CONV / POOL output modes, as lrcn_debug_conv_gemm (include/lrcn_gemm_debug.h) launches it.  The two regimes
are gemm_ref's, whose constants, bits() and chunk() are reused; the reference is a float64 cross-correlation of the operand values the
kernel actually receives (the host tensors are made in the element type first), then the bias, then the ReLU, then the 2x2 maximum, then
ONE torch cast to bf16 for a bf16 output.  Rounding commutes with the maximum because it is monotone.

(a) Integer regime, expected bit for bit.  Every partial sum of any subset of the terms is an integer of magnitude at most
    9 Cin max|x| max|w| + max|bias| < 2^24 (asserted), so any tile shape, tap order, K split or slab order gives exactly the integer
    result.  As in gemm_ref at least half of the values the kernel WRITES (after ReLU and maximum) exceed 2^8 in magnitude and some exceed
    2^11, so a bf16 slab or a truncating conversion cannot pass; a ReLU case carries a bias offset to get there (operands in [-8, 8]
    without one: 40 % above 2^8), and both signs occur before the ReLU.

(b) Real-valued regime, bound derived: gemm_ref's (K + 34) 2^-24 (|x| * |w| + |bias|) with K = 9 Cin, plus 2^-8 |ref| for a bf16 output.
    ReLU and the maximum are 1-Lipschitz; a pooled output takes the largest bound of its window's four pixels.

Layout (`Problem`): x, w and y are sub-views of larger flat allocations at a 16-byte aligned, not page aligned, offset.  x has at least
(W + 1) Cin + 64 elements of 2^15 on both sides -- the 3x3 taps of the first and last image rows point that far outside the tensor, the
engines mask them, and a wrong mask reads a loud finite value from memory the test owns.  w has a lead-in and a guard row of 2^15.  y's
padding columns (ldc > Cout in some cases), guard row and lead-in hold C_SENTINEL and must come back bit for bit; its interior starts
as C_STALE.
"""
import functools
import zlib

import numpy as np
import torch

from gemm_ref import BF16, C_SENTINEL, C_STALE, F32, MAX_SLICES, OPERAND_PAD, _int_magnitude, _torch_type, bits, chunk  # noqa: F401

P8F = {"LRCN_8P": "force"}
NOGLDS = {"LRCN_GLDS": "0"}
GLDSF = {"LRCN_GLDS": "force", "LRCN_8P": "0"}
LEAD = 3   # chunks of lead-in before w and y (x's lead-in is its tap margin)


class Case:
    """One case: the geometry (W x H x images, Cin -> Cout), the epilogue, the knobs and the route string the router must report."""

    def __init__(self, route, W, H, N, Cin, Cout, dtype=BF16, relu=False, pool=False, pad_c=0, wg_cap=0, env=None, regime="int", tag=""):
        self.route, self.W, self.H, self.N, self.Cin, self.Cout, self.dtype = route, W, H, N, Cin, Cout, dtype
        self.relu, self.pool, self.pad_c, self.wg_cap = relu, pool, pad_c, wg_cap
        self.bias = relu or regime == "real"   # a ReLU case carries a bias: its offset keeps half of the outputs above 2^8
        self.env = dict(env or {})
        self.regime, self.tag = regime, tag

    @property
    def M(self):
        return self.N * self.H * self.W

    @property
    def K(self):
        return 9 * self.Cin

    @property
    def out_rows(self):
        return self.M // 4 if self.pool else self.M

    @property
    def ldc(self):
        return self.Cout + self.pad_c * chunk(self.dtype)

    @property
    def operands_key(self):
        """What x, w and the bias-free convolution depend on: the variants of one table row share them."""
        return (self.W, self.H, self.N, self.Cin, self.Cout, self.dtype, self.regime)

    @property
    def id(self):
        parts = [self.route.replace(":", "_"), "%dx%dx%d" % (self.W, self.H, self.N), "%dto%d" % (self.Cin, self.Cout),
                 "f32" if self.dtype == F32 else "bf16"]
        if self.relu:
            parts.append("relu")
        if self.pool:
            parts.append("pool")
        if self.pad_c:
            parts.append("ldc+%d" % (self.pad_c * chunk(self.dtype)))
        if self.wg_cap:
            parts.append("cap%d" % self.wg_cap)
        if self.regime != "int":
            parts.append(self.regime)
        if self.tag:
            parts.append(self.tag)
        return "-".join(parts)


def _table():
    c = []

    def row(route, W, H, N, Cin, Cout, r=False, **k):
        """Every row runs with the maximum off and on; a row marked r also with a ReLU and a bias."""
        for relu in ((False, True) if r else (False,)):
            for pool in (False, True):
                c.append(Case(route, W, H, N, Cin, Cout, relu=relu, pool=pool, **k))

    def one(route, W, H, N, Cin, Cout, **k):
        for pool in (False, True):
            c.append(Case(route, W, H, N, Cin, Cout, pool=pool, **k))

    # ---- 8p, 256 x 128 tiles (forced below the grid threshold)
    row("8p:1", 16, 16, 1, 64, 128, env=P8F)                       # one whole tile; every border pixel
    row("8p:1", 12, 20, 3, 128, 200, r=True, env=P8F)              # W != H, a row tail (720 rows), a column tail, image seams inside a tile
    row("8p:1", 12, 20, 3, 128, 196, r=True, env=P8F)              # Cout % 8 != 0: the direct stores
    one("8p:1", 12, 20, 3, 128, 200, relu=True, pad_c=1, env=P8F)  # ldc = Cout + 8: padding columns beside a column tail
    # ---- 8p, 256 x 256 tiles
    row("8p:0", 16, 16, 1, 64, 256, env=P8F)                       # one whole tile
    row("8p:0", 10, 14, 5, 192, 520, r=True, env=P8F)              # three channel slices times nine taps; every tail
    # ---- 8p under a cap: the persistent walk (tiles w, w + G, ... with the next tile's first K-tile issued early)
    row("8p:0", 16, 16, 12, 64, 256, env=P8F, wg_cap=8)            # 12 tiles on 8 workgroups
    row("8p:1", 14, 14, 13, 128, 320, r=True, env=P8F, wg_cap=8)   # 30 tiles on 8 workgroups: four rounds, the last row tile partial
    # ---- 8p, 512 x 128 tiles: only from 400 row tiles, no knob
    row("8p:2", 16, 16, 799, 64, 128, r=True)                      # 204544 rows = 400 tiles of 512, the last half full
    one("8p:2", 16, 16, 799, 64, 128, relu=True, wg_cap=64)        # ... walked by 64 workgroups
    row("8p:1", 16, 16, 798, 64, 128)                              # one tile fewer: 798 tiles of 256 x 128
    # ---- 8p-splitk, no knob: conv5's geometry at a decode batch
    row("8p-splitk:6", 14, 14, 8, 512, 512, r=True)                # 28 tiles x 6 slices of 12 K-tiles
    one("8p-splitk:6", 14, 14, 8, 512, 512, relu=True, wg_cap=8)   # 28 tiles walked under split-K
    row("8p-splitk:6", 16, 16, 4, 512, 512)                        # exactly LRCN_8P_SPLITK_MIN's 96 workgroups
    row("glds-small", 16, 16, 4, 512, 512, env={"LRCN_8P_SPLITK": "0"})   # the split-K form off: 64 tiles of 128 x 64, below glds's 96
    # ---- 8p-splitk with two slices: 27 K-tiles cut 13 + 14, the seam inside channel slice 1; a row tail; pooled 7 x 7
    row("8p-splitk:2", 14, 14, 2, 192, 136, r=True, env={"LRCN_8P_SPLITK_MIN": "1"})
    row("8p-splitk:2", 12, 20, 2, 192, 132, r=True, env={"LRCN_8P_SPLITK_MIN": "1"})   # W != H and Cout % 8 != 0 in the reduce kernel
    # ---- glds forced, bf16, every tile config through choose_cfg's rules (the route string does not carry the tile)
    row("glds", 16, 16, 100, 64, 512, env=GLDSF, tag="256x256")    # 100 x 2 = 200 workgroups
    row("glds", 16, 16, 100, 64, 256, env=GLDSF, tag="256x128")    # 100 x 2
    row("glds", 16, 16, 100, 64, 128, env=GLDSF, tag="256x64")     # 100 x 2
    row("glds", 12, 20, 3, 128, 72, r=True, env=GLDSF, tag="128x64")
    row("glds", 12, 20, 3, 128, 136, r=True, env=GLDSF, tag="128x64")   # row and column tails
    # ---- glds-small, no knob
    row("glds-small", 16, 16, 4, 64, 128)                          # 16 workgroups: the rung's floor
    row("glds-small", 12, 20, 5, 64, 136, r=True)
    row("glds-small", 12, 20, 5, 32, 136, r=True, dtype=F32)
    # ---- glds, f32: the exact-fp32 stack's default route, each tile
    row("glds", 16, 16, 100, 32, 512, dtype=F32, tag="256x256")
    row("glds", 16, 16, 100, 32, 256, dtype=F32, tag="256x128")
    row("glds", 16, 16, 100, 32, 128, dtype=F32, tag="256x64")
    row("glds", 12, 20, 3, 96, 72, r=True, dtype=F32, env={"LRCN_GLDS": "force"}, tag="128x64")
    # ---- gemm_nt, 64 x 64 tiles
    row("gemm_nt", 6, 10, 2, 64, 72, r=True)                       # 120 rows: below every other engine
    row("gemm_nt", 6, 10, 2, 32, 72, r=True, dtype=F32)
    row("gemm_nt", 12, 20, 3, 128, 136, env=NOGLDS)
    row("gemm_nt", 12, 20, 3, 96, 136, dtype=F32, env=NOGLDS)
    # ---- gemm_nt, 128 x 128 tiles: from 160 of them
    row("gemm_nt", 16, 16, 40, 64, 256, env=NOGLDS, tag="128x128")             # exactly 160 tiles
    row("gemm_nt", 12, 20, 43, 64, 200, r=True, env=NOGLDS, tag="128x128")     # 81 x 2 tiles, row and column tails
    row("gemm_nt", 16, 16, 40, 32, 256, dtype=F32, env=NOGLDS, tag="128x128")
    # ---- real-valued regime: each listed route, both output modes
    one("8p:0", 10, 14, 5, 192, 520, env=P8F, regime="real")
    one("8p:1", 12, 20, 3, 128, 200, env=P8F, regime="real", relu=True)
    one("8p-splitk:2", 14, 14, 2, 192, 136, env={"LRCN_8P_SPLITK_MIN": "1"}, regime="real")
    one("glds", 12, 20, 3, 128, 136, env=GLDSF, regime="real", relu=True, tag="128x64")
    one("glds-small", 12, 20, 5, 32, 136, dtype=F32, regime="real")
    one("gemm_nt", 6, 10, 2, 64, 72, regime="real")
    one("gemm_nt", 12, 20, 3, 96, 136, dtype=F32, env=NOGLDS, regime="real", relu=True)
    return c


CASES = _table()
# every rung of gemm_route.hip's ladder that has a CONV3 mode for bf16 / f32; "8p:2" is the one rung allowed one shape plus its capped run
RUNGS = ("8p:0", "8p:1", "8p:2", "8p-splitk", "glds", "glds-small", "gemm_nt")
REAL_ROUTES = ("8p:0", "8p:1", "8p-splitk", "glds", "glds-small", "gemm_nt")


def x_margin(cs):
    """Elements of 2^15 before and behind x: at least (W + 1) Cin + 64, in whole 16-byte chunks, and not a whole number of pages."""
    ce = chunk(cs.dtype)
    m = ((cs.W + 1) * cs.Cin + 64 + ce - 1) // ce * ce
    if (m * 16 // ce) % 4096 == 0:
        m += ce
    return m


def conv_taps(x, w):
    """float64 3x3 cross-correlation: x [N][H][W][Cin], w [Cout][9][Cin] (float64 tensors) -> [N][H][W][Cout], one product per tap."""
    N, H, W, Cin = x.shape
    xp = torch.zeros(N, H + 2, W + 2, Cin, dtype=torch.float64)
    xp[:, 1:H + 1, 1:W + 1] = x
    out = torch.zeros(N * H * W, w.shape[0], dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            out += xp[:, kh:kh + H, kw:kw + W].reshape(N * H * W, Cin) @ w[:, kh * 3 + kw, :].T
    return out.view(N, H, W, w.shape[0])


def pool2(t):
    """2x2 windows of [N][H][W][C] -> [N][H/2][W/2][C] by their maximum."""
    N, H, W, C = t.shape
    return t.view(N, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))


@functools.lru_cache(maxsize=1)
def _operands(key, seed):
    """x, w in the element type and their bias-free float64 convolution (and, real-valued regime, that of their magnitudes): computed once
    per table row and shared, read-only, among its variants."""
    W, H, N, Cin, Cout, dtype, regime = key
    rng = np.random.default_rng(seed)
    t = _torch_type(dtype == F32)
    if regime == "int":
        a = _int_magnitude(9 * Cin)
        x = torch.from_numpy(rng.integers(-a, a + 1, size=(N, H, W, Cin)).astype(np.float32)).to(t)
        w = torch.from_numpy(rng.integers(-a, a + 1, size=(Cout, 9, Cin)).astype(np.float32)).to(t)
        mag = None
    else:
        a = None
        x = torch.from_numpy(rng.standard_normal((N, H, W, Cin)).astype(np.float32)).to(t)
        w = torch.from_numpy(rng.standard_normal((Cout, 9, Cin)).astype(np.float32)).to(t)
        mag = conv_taps(x.double().abs(), w.double().abs())
    return x, w, conv_taps(x.double(), w.double()), mag, a


class Problem:
    """Host operands of one case in their element type, laid out with margins, guard rows and lead-ins, and the float64 reference."""

    def __init__(self, case):
        cs = self.case = case
        ce = chunk(cs.dtype)
        t = _torch_type(cs.dtype == F32)
        key = cs.operands_key
        x, w, conv, mag, a = _operands(key, zlib.crc32(repr(key).encode()))
        self.amax = a
        rng = np.random.default_rng(zlib.crc32(cs.id.encode()))

        if not cs.bias:
            bias = None
        elif cs.regime == "int":
            # a ReLU case: the bias carries an offset of ~0.75 sigma (sigma of an interior pixel's sum), so that the ReLU cuts about a
            # quarter of the outputs and the median of the rest stays above 2^8; bf16-exact integers (multiples of 16 below 2^12)
            sigma = np.sqrt(cs.K) * a * (a + 1) / 3.0
            boff = min(int(0.75 * sigma) // 16 * 16, 2048)
            bias = (boff + 16 * rng.integers(-8, 9, size=cs.Cout)).astype(np.float32)
        else:
            bias = rng.standard_normal(cs.Cout).astype(np.float32)
        self.bias = torch.from_numpy(bias) if cs.bias else None

        # ---- layout
        self.xm = x_margin(cs)
        self.x_flat = torch.full((2 * self.xm + x.numel(),), OPERAND_PAD, dtype=t)
        self.x = self.x_flat[self.xm:self.xm + x.numel()].view(x.shape)
        self.x.copy_(x)
        self.off_w = self.off_c = LEAD * ce
        self.w_flat = torch.full((self.off_w + (cs.Cout + 1) * cs.K,), OPERAND_PAD, dtype=t)
        self.w = self.w_flat[self.off_w:].view(cs.Cout + 1, 9, cs.Cin)
        self.w[:cs.Cout].copy_(w)
        self.y_flat = torch.full((self.off_c + (cs.out_rows + 1) * cs.ldc,), C_SENTINEL, dtype=t)
        self.y = self.y_flat[self.off_c:].view(cs.out_rows + 1, cs.ldc)
        self.y[:cs.out_rows, :cs.Cout] = C_STALE

        # ---- the reference, from the values in the tensors above (after their rounding to the element type)
        b64 = self.bias.double() if cs.bias else torch.zeros(cs.Cout, dtype=torch.float64)
        self.pre = conv + b64   # [N][H][W][Cout], before the ReLU
        ref = self.pre.clamp_min(0.0) if cs.relu else self.pre
        if cs.pool:
            ref = pool2(ref)
        self.ref = ref.reshape(cs.out_rows, cs.Cout).numpy()
        if cs.regime == "int":
            self.check_int_conditions(x, w, b64)
            exp = torch.from_numpy(self.ref).to(torch.float32)   # exact: integers below 2^24
            self.expected = exp if cs.dtype == F32 else exp.to(torch.bfloat16)   # ONE round-to-nearest-even
        else:
            bound = (cs.K + MAX_SLICES + 2) * 2.0 ** -24 * (mag + b64.abs())
            if cs.dtype == BF16:
                bound = bound + 2.0 ** -8 * (self.pre.clamp_min(0.0) if cs.relu else self.pre).abs()
            if cs.pool:
                bound = pool2(bound)   # the largest bound of the window's four pixels
            self.bound = bound.reshape(cs.out_rows, cs.Cout).numpy()

    def check_int_conditions(self, x, w, b64):
        """Conditions on the INPUTS of an integer-regime case (not tolerances): headroom below 2^24, and written values large enough to
        tell a bf16 intermediate from an f32 one."""
        cs = self.case
        pre = self.pre.numpy()
        for v in (x.double().numpy(), w.double().numpy(), b64.numpy(), pre):
            assert np.array_equal(v, np.rint(v)), "integer regime: a non-integer value"
        head = 9 * cs.Cin * float(x.abs().max()) * float(w.abs().max()) + float(b64.abs().max())
        assert head < 2 ** 24, (cs.id, head)
        assert (pre < 0).any() and (pre > 0).any(), (cs.id, "both signs must occur before the ReLU")
        if cs.relu:
            cut = float((pre < 0).mean())
            assert cut >= 0.05, (cs.id, "ReLU cuts only %.3f of the outputs" % cut)
        big = np.abs(self.ref)   # the tensor the kernel writes
        assert (big > 2 ** 8).mean() >= 0.5, (cs.id, "share above 2^8: %.3f" % (big > 2 ** 8).mean())
        assert (big > 2 ** 11).any(), (cs.id, "nothing above 2^11")


def where(cs, rows):
    """(image, y, x) of output rows of y (its pooled rows when cs.pool) -- for failure reports."""
    W, H = (cs.W // 2, cs.H // 2) if cs.pool else (cs.W, cs.H)
    rows = np.asarray(rows)
    return rows // (H * W), rows // W % H, rows % W
