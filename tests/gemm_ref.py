"""Exact host references and the case table of the plain GEMM engine tests (tests only; no GPU, nothing of the code under test).

C[M][N] (+)= A[M][K] B[N][K]^T (+ bias) (ReLU), the contraction of csrc/gemm.h in PLAIN mode.  Both regimes compute the reference in float64
from the operand values the kernel actually receives: the host tensors are made in the element type first (torch.bfloat16 / float32), and
the same tensors go to the device and, widened to float64, into the reference.

(a) Integer regime, expected bit for bit.  A, B, bias and the prior contents of C are small integers, exact in bf16.  With
    K max|a| max|b| + max|bias| + max|C0| < 2^24 every partial sum of every subset of the terms is an integer below 2^24, which f32 holds
    exactly: whatever the tile shape, the K split, the slab order or the order of float atomics, an engine that adds the right terms once
    each returns exactly the integer result.  The expected C is that integer (a float64 matmul of integers below 2^24 is itself exact, as
    checked), then max(., 0) under ReLU, then ONE round-to-nearest-even to bf16 for a bf16 output (torch's own float32 -> bfloat16 cast).
    So that a slab or accumulator kept in bf16, or a truncating output conversion, cannot pass unseen, at least half of the expected values
    exceed 2^8 in magnitude and some exceed 2^11 (integers up to 256 survive bf16 unchanged and would prove nothing).  Both conditions are
    asserted on the inputs by `Problem`, and both signs must occur before the ReLU.

(b) Real-valued regime, bound derived.  A, B standard normal, rounded to the operand type; the reference is the float64 product of the
    rounded operands.  f32 accumulation of K + 2 terms in any order over at most S = 32 K-slices is bounded elementwise by
    (K + S + 2) 2^-24 (|A| |B|^T + |bias| + |C0|); a bf16 output adds one rounding, 2^-8 |ref|.

Operand layout (`Problem`): every matrix is a sub-view of a larger flat allocation, `off` elements in (16-byte aligned, not page aligned),
with leading dimension K or N plus padding and one guard row behind the last row.  The operands' padding and guard hold 2^15 -- finite,
exact in bf16, and large enough that reading ONE such element breaks exactness (NaN would not do: 0 * NaN would also trip an engine that
legitimately multiplies padding by zero rows).  C's padding, guard row and lead-in hold a sentinel that must come back bit for bit.
"""
import zlib

import numpy as np
import torch

F32, BF16 = 0, 1   # LRCN_F32, LRCN_BF16
MAX_SLICES = 32    # the largest K-slice count a planner allows (gemm_skinny_splitk)
OPERAND_PAD = float(2 ** 15)
C_SENTINEL = -12288.0   # exact in bf16 and f32; C's padding, guard row and lead-in (compared apart from the interior, bit for bit)
C_STALE = 768.0         # what C's interior holds before a call that must overwrite it (neither beta nor c_is_zero)


class Case:
    """One row of the table: the shape, the knobs, the router inputs and the route string the router must report."""

    def __init__(self, route, M, N, K, dtype=BF16, c_f32=False, bias=False, relu=False, beta=False, c_is_zero=False, det=False, pad_a=0,
                 pad_b=0, pad_c=0, off=0, free_cus=0, bg_cus=0, wg_cap=0, env=None, regime="int", amax=None, tag=""):
        self.route, self.M, self.N, self.K, self.dtype = route, M, N, K, dtype
        self.c_f32 = bool(c_f32) or dtype == F32
        self.bias, self.relu, self.beta, self.c_is_zero, self.det = bias, relu, beta, c_is_zero, det
        self.pad_a, self.pad_b, self.pad_c, self.off = pad_a, pad_b, pad_c, off   # in 16-byte chunks
        self.free_cus, self.bg_cus, self.wg_cap = free_cus, bg_cus, wg_cap
        self.env = dict(env or {})
        self.regime, self.amax, self.tag = regime, amax, tag
        assert not relu or bias, "a ReLU case carries a bias: its offset keeps half of the outputs above 2^8"

    def leading_dims(self):
        """(lda, ldb, ldc) in elements: K rounded up to whole 16-byte chunks, N as it is, plus the case's padding chunks."""
        ce, cc = chunk(self.dtype), (4 if self.c_f32 else 8)
        kc = (self.K + ce - 1) // ce * ce
        return kc + self.pad_a * ce, kc + self.pad_b * ce, self.N + self.pad_c * cc

    @property
    def id(self):
        parts = [self.route.replace(":", "_"), "%dx%dx%d" % (self.M, self.N, self.K), "f32" if self.dtype == F32 else "bf16"]
        if self.dtype == BF16 and self.c_f32:
            parts.append("cf32")
        for flag in ("bias", "relu", "beta"):
            if getattr(self, flag):
                parts.append(flag)
        if self.c_is_zero:
            parts.append("czero")
        if self.det:
            parts.append("det")
        if self.pad_a or self.pad_b or self.pad_c:
            parts.append("pad%d.%d.%d" % (self.pad_a, self.pad_b, self.pad_c))
        if self.off:
            parts.append("off%d" % self.off)
        if self.regime != "int":
            parts.append(self.regime)
        if self.tag:
            parts.append(self.tag)
        return "-".join(parts)


P8F = {"LRCN_8P": "force"}
NOGLDS = {"LRCN_GLDS": "0"}
GLDSF = {"LRCN_GLDS": "force", "LRCN_8P": "0"}   # glds wherever it is eligible; 8p off so that its rungs do not take the large grids first
ODD = 37   # "a large odd number of chunks" of padding


def _table():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))   # noqa: E731
    # ---- 8p, 256 x 256 tiles (forced below the grid threshold)
    add("8p:0", 256, 256, 128, env=P8F)                                            # exactly two K-tiles, one whole tile
    add("8p:0", 300, 520, 192, env=P8F, bias=True, relu=True, pad_a=1, pad_b=ODD, pad_c=1, off=3)   # staged bf16 epilogue, every tail
    add("8p:0", 513, 768, 320, env=P8F, c_f32=True, beta=True, pad_c=ODD, off=1)   # one row past two tiles; direct f32 epilogue
    add("8p:0", 300, 520, 192, env=P8F, beta=True, bias=True, pad_a=ODD, pad_c=1)  # bf16 accumulate: leaves the staged epilogue
    add("8p:0", 300, 516, 128, env=P8F, bias=True, relu=True, pad_c=1)             # N % 8 != 0: bf16 output through the direct stores
    add("8p:0", 300, 520, 192, env=P8F, bias=True, regime="real")
    # ---- 8p, 256 x 128 tiles
    add("8p:1", 256, 128, 128, env=P8F, bias=True)
    add("8p:1", 300, 200, 256, env=P8F, c_f32=True, bias=True, relu=True, pad_a=1, pad_b=1, pad_c=ODD, off=5)
    add("8p:1", 700, 384, 192, env=P8F, beta=True, pad_b=ODD, off=2)
    add("8p:1", 700, 384, 192, env=P8F, c_f32=True, bias=True, regime="real")
    # ---- 8p without a knob: a grid of >= 128 tiles
    add("8p:1", 2048, 4096, 128, bias=True, relu=True)                             # 128 tiles of 256 x 256 are < 200, 256 of 256 x 128 are not
    add("8p:0", 2560, 5120, 128, c_f32=True, beta=True)                            # 200 tiles of 256 x 256
    # ---- 8p, 512 x 128 tiles: only from 400 row tiles
    add("8p:2", 204300, 128, 128, bias=True)
    # ---- 8p-bg: beside the capped convolution grids, 256 .. 512 rows, N >= 512
    add("8p-bg:1", 300, 520, 256, bg_cus=32, bias=True, relu=True, pad_a=1, pad_c=1, off=1)
    add("8p-bg:1", 512, 1024, 128, bg_cus=32, c_f32=True, beta=True)
    add("8p-bg:1", 256, 512, 128, bg_cus=32)                                        # the window's lower edge
    add("8p-bg:1", 512, 1024, 128, bg_cus=32, wg_cap=8, c_f32=True, bias=True, tag="walk")   # 16 tiles on 8 persistent workgroups
    add("glds-small", 513, 1024, 128, bg_cus=32, bias=True)                         # one row past the window: another rung
    # ---- skinny: M <= 128, the four row-count instantiations (<= 32, <= 64, <= 128 rows; 129 .. 256 under skinny-last)
    add("skinny", 1, 16, 64, amax=128)
    add("skinny", 16, 64, 64, bias=True, relu=True, amax=64)
    add("skinny", 17, 80, 2048, c_f32=True, beta=True, pad_a=1, pad_b=1, pad_c=1, off=1)
    add("skinny", 32, 200, 64, bias=True, pad_c=ODD)
    add("skinny", 33, 72, 64, c_f32=True, bias=True, relu=True, pad_a=ODD)
    add("skinny", 64, 50, 2048, beta=True, pad_b=ODD, pad_c=1)                      # N % 16 != 0 and N % 4 != 0
    add("skinny", 65, 200, 64, c_f32=True, off=7)
    add("skinny", 128, 80, 2048, bias=True, relu=True, pad_a=1, pad_b=1, pad_c=1)
    add("skinny", 8, 64, 8192, bias=True, relu=True, tag="split8")                  # its own split-K: 8 slabs, the shared reduce kernel
    add("skinny", 40, 100, 4096, c_f32=True, beta=True, bias=True, pad_c=1, tag="split4")   # split-K with a column tail inside a workgroup
    add("skinny", 8, 66, 8192, bias=True, tag="nosplit")                            # N % 4 != 0: the split-K must stand down
    add("skinny", 40, 100, 4096, beta=True, pad_c=ODD, pad_a=1, tag="split4")       # the reduce kernel's bf16 accumulate
    add("skinny", 33, 72, 64, c_f32=True, bias=True, regime="real")
    add("skinny", 8, 64, 8192, bias=True, regime="real", tag="split8")
    # ---- skinny-last: 128 < M <= 256 with too few tiles for the rungs above
    add("skinny-last", 200, 512, 128, bias=True, relu=True, pad_a=1, pad_c=1)
    add("skinny-last", 256, 320, 64, c_f32=True, beta=True, pad_b=1, off=3)
    add("skinny-last", 200, 512, 2048, bias=True, tag="split2")                     # two slabs
    add("skinny-last", 129, 52, 64, c_f32=True, bias=True, pad_c=1)
    # ---- 8p-splitk:S
    add("8p-splitk:10", 300, 640, 5120, beta=True, pad_a=1, pad_b=1, pad_c=1, off=1)
    add("8p-splitk:10", 300, 640, 5120, c_f32=True, bias=True, relu=True, pad_c=ODD)
    add("8p-splitk:16", 256, 1024, 8192, bias=True, relu=True)                      # bf16 output
    add("8p-splitk:12", 256, 1024, 8192, free_cus=96, c_f32=True, beta=True, bias=True)   # 96 free CUs: 12 slices instead of 16
    add("8p-splitk:10", 300, 644, 5120, c_f32=True, bias=True, pad_c=1)             # N % 8 != 0 (N % 4 == 0): slab rows of 644 floats
    add("8p-splitk:10", 300, 640, 5120, c_f32=True, bias=True, regime="real")
    add("glds-small", 300, 640, 5120, env={"LRCN_8P_SPLITK": "0"}, bias=True)       # the split-K form off: the next rung that fits
    add("glds-small", 300, 640, 5120, env={"LRCN_8P_SPLITK_MIN": "101"}, beta=True)   # 100 workgroups are one too few
    # ---- glds: the grid fills the chip
    add("glds", 1536, 1024, 128, bias=True, relu=True)                              # 192 tiles of 128 x 64
    add("glds", 300, 512, 2048, c_f32=True, bias=True, tag="atomic8")               # 24 tiles x 8 K-slices by float atomics
    add("glds", 300, 512, 2048, c_f32=True, beta=True, bias=True, pad_c=1, tag="atomic8")
    # ---- glds forced, every tile config through choose_cfg's rules
    add("glds", 2400, 5100, 128, env=GLDSF, bias=True, relu=True, tag="256x256")    # 10 x 20 tiles of 256 x 256
    add("glds", 1200, 5000, 64, env=GLDSF, c_f32=True, beta=True, tag="256x128")    # 5 x 40 of 256 x 128
    add("glds", 1200, 2500, 64, env=GLDSF, bias=True, pad_a=1, pad_b=1, pad_c=1, off=1, tag="256x64")   # 5 x 40 of 256 x 64
    add("glds", 129, 72, 128, env=GLDSF, bias=True, relu=True, pad_c=ODD, tag="128x64")
    add("glds", 129, 72, 128, env=GLDSF, c_f32=True, beta=True, pad_a=ODD, pad_b=1, tag="128x64")
    add("glds", 1200, 2500, 64, env=GLDSF, c_f32=True, bias=True, regime="real", tag="256x64")
    # ---- glds-small
    add("glds-small", 300, 512, 128, bias=True, relu=True, pad_a=1, pad_b=ODD, pad_c=1, off=1)
    add("glds-small", 300, 512, 512, c_f32=True, bias=True, tag="atomic2")          # 24 tiles x 2 K-slices by float atomics; memset first
    add("glds-small", 300, 512, 512, c_f32=True, bias=True, c_is_zero=True, tag="atomic2")   # ... the caller vouches for the zeros
    add("glds-small", 300, 512, 512, c_f32=True, beta=True, pad_c=1, tag="atomic2")
    add("glds-small", 300, 512, 512, c_f32=True, bias=True, det=True)               # deterministic: the route stays, the split goes
    add("glds-small", 300, 512, 2048, c_f32=True, bias=True, det=True)              # ("glds" with its 8 slices otherwise: see above)
    add("glds-small", 300, 512, 512, c_f32=True, bias=True, pad_c=1)                # ldc != N without beta: no split either
    add("glds-small", 300, 512, 512, c_f32=True, bias=True, regime="real", tag="atomic2")
    # ---- gemm_nt: f32, and bf16 where no other engine fits
    add("gemm_nt", 1, 8, 4, dtype=F32, amax=256)
    add("gemm_nt", 1, 8, 8, amax=256)
    add("gemm_nt", 130, 100, 96, bias=True, relu=True, pad_a=1, pad_b=1, pad_c=1, off=1)
    add("gemm_nt", 130, 100, 72, beta=True, tag="ld72")                             # K = lda = ldb = 72: not a multiple of 64
    add("gemm_nt", 130, 100, 70, c_f32=True, bias=True, pad_a=ODD, tag="ktail")     # K % 8 != 0: the last chunk is masked, its tail is padding
    add("gemm_nt", 300, 512, 128, env=NOGLDS, bias=True, relu=True, pad_c=ODD)      # every direct-to-LDS engine off
    add("gemm_nt", 64, 64, 64, env=NOGLDS, c_f32=True, beta=True)
    add("gemm_nt", 300, 200, 100, dtype=F32, bias=True, relu=True, pad_a=1, pad_b=ODD, pad_c=1, off=1)
    add("gemm_nt", 256, 1024, 8192, dtype=F32, beta=True)
    add("gemm_nt", 65, 33, 30, dtype=F32, bias=True, pad_a=1, tag="ktail")          # K % 4 != 0
    add("gemm_nt", 1300, 1900, 36, dtype=F32, bias=True, relu=True, pad_c=1, tag="128x128")   # 11 x 15 = 165 tiles: the 128 x 128 config
    add("gemm_nt", 1300, 1900, 40, beta=True, bias=True, tag="128x128")
    add("gemm_nt", 300, 200, 100, dtype=F32, bias=True, regime="real")
    add("gemm_nt", 130, 100, 96, bias=True, regime="real")
    return c


CASES = _table()
# every rung of gemm_route.hip's ladder that has a PLAIN mode; "8p:2" is the one rung allowed a single case
RUNGS = ("8p:0", "8p:1", "8p:2", "8p-bg", "skinny", "8p-splitk", "glds", "skinny-last", "glds-small", "gemm_nt")


def chunk(dtype):
    return 8 if dtype == BF16 else 4   # elements per 16-byte chunk


def _torch_type(is_f32):
    return torch.float32 if is_f32 else torch.bfloat16


def _int_magnitude(K):
    """Largest |a| = |b| of a case: sigma of one result ~ sqrt(K) a (a + 1) / 3 (uniform integers in [-a, a]) should reach ~1500, so that
    most results exceed 2^8 and one in six 2^11, within K a^2 < 2^23."""
    a = 1
    while np.sqrt(K) * a * (a + 1) / 3.0 < 1500.0 and a < 256 and K * (a + 1) ** 2 < 2 ** 23:
        a += 1
    return a


class Problem:
    """Host operands of one case in their element type, laid out with padding, guard rows and a lead-in, and the float64 reference."""

    def __init__(self, case, seed=None):
        cs = self.case = case
        rng = np.random.default_rng(zlib.crc32(cs.id.encode()) if seed is None else seed)
        M, N, K = cs.M, cs.N, cs.K
        ce, cc = chunk(cs.dtype), (4 if cs.c_f32 else 8)
        self.lda, self.ldb, self.ldc = cs.leading_dims()
        self.off_ab, self.off_c = cs.off * ce, cs.off * cc
        op_t, c_t = _torch_type(cs.dtype == F32), _torch_type(cs.c_f32)

        if cs.regime == "int":
            a = cs.amax or _int_magnitude(K)
            self.amax = self.bmax = a
            sigma = np.sqrt(K) * a * (a + 1) / 3.0
            A = rng.integers(-a, a + 1, size=(M, K)).astype(np.float32)
            B = rng.integers(-a, a + 1, size=(N, K)).astype(np.float32)
            # a ReLU case: the bias carries an offset of ~0.75 sigma, so that ReLU cuts about a quarter of the outputs and the median of
            # the rest stays above 2^8; bf16-exact integers (multiples of 16 below 2^12)
            boff = min(int(0.75 * sigma) // 16 * 16, 2048) if cs.relu else 0
            bias = (boff + 16 * rng.integers(-8, 9, size=N)).astype(np.float32) if cs.bias else None
            C0 = rng.integers(-200, 201, size=(M, N)).astype(np.float32) if cs.beta else None
        else:
            self.amax = self.bmax = None
            A = rng.standard_normal((M, K)).astype(np.float32)
            B = rng.standard_normal((N, K)).astype(np.float32)
            bias = rng.standard_normal(N).astype(np.float32) if cs.bias else None
            C0 = rng.standard_normal((M, N)).astype(np.float32) if cs.beta else None

        def lay(values, rows, cols, ld, off, t, pad, guard_rows=1):
            flat = torch.full((off + (rows + guard_rows) * ld,), pad, dtype=t)
            view = flat[off:].view(rows + guard_rows, ld)
            view[:rows, :cols] = torch.from_numpy(values).to(t)
            return flat, view

        self.A_flat, self.A = lay(A, M, K, self.lda, self.off_ab, op_t, OPERAND_PAD)
        self.B_flat, self.B = lay(B, N, K, self.ldb, self.off_ab, op_t, OPERAND_PAD)
        interior = C0 if cs.beta else np.full((M, N), 0.0 if cs.c_is_zero else C_STALE, np.float32)
        self.C_flat, self.C = lay(interior, M, N, self.ldc, self.off_c, c_t, C_SENTINEL)
        self.bias = torch.from_numpy(bias) if cs.bias else None

        # ---- the reference, from the values in the tensors above (after their rounding to the element type)
        A64 = self.A[:M, :K].double().numpy()
        B64 = self.B[:N, :K].double().numpy()
        b64 = self.bias.double().numpy() if cs.bias else np.zeros(N)
        c64 = self.C[:M, :N].double().numpy() if cs.beta else np.zeros((M, N))
        self.pre = A64 @ B64.T + b64[None, :] + c64   # before the ReLU
        ref = np.maximum(self.pre, 0.0) if cs.relu else self.pre
        self.ref = ref
        if cs.regime == "int":
            self.check_int_conditions(A64, B64, b64, c64)
            exp = torch.from_numpy(ref).to(torch.float32)   # exact: integers below 2^24
            self.expected = exp if cs.c_f32 else exp.to(torch.bfloat16)   # ONE round-to-nearest-even
        else:
            mag = np.abs(A64) @ np.abs(B64).T + np.abs(b64)[None, :] + np.abs(c64)
            self.bound = (K + MAX_SLICES + 2) * 2.0 ** -24 * mag
            if not cs.c_f32:
                self.bound = self.bound + 2.0 ** -8 * np.abs(ref)

    def check_int_conditions(self, A64, B64, b64, c64):
        """Conditions on the INPUTS of an integer-regime case (not tolerances): headroom below 2^24, and results large enough to tell a
        bf16 intermediate from an f32 one."""
        cs, K = self.case, self.case.K
        for x in (A64, B64, b64, c64, self.pre):
            assert np.array_equal(x, np.rint(x)), "integer regime: a non-integer value"
        head = K * np.abs(A64).max() * np.abs(B64).max() + np.abs(b64).max() + np.abs(c64).max()
        assert head < 2 ** 24, (cs.id, head)
        assert np.abs(self.pre).max() < 2 ** 24   # (implied; the float64 product itself is exact far beyond)
        assert (self.pre < 0).any() and (self.pre > 0).any(), (cs.id, "both signs must occur before the ReLU")
        if cs.relu:
            cut = float((self.pre < 0).mean())
            assert cut >= 0.05, (cs.id, "ReLU cuts only %.3f of the outputs" % cut)
        big = np.abs(self.ref)
        assert (big > 2 ** 8).mean() >= 0.5, (cs.id, "share above 2^8: %.3f" % (big > 2 ** 8).mean())
        assert (big > 2 ** 11).any(), (cs.id, "nothing above 2^11")


def bits(t):
    """The tensor's bit pattern as a numpy integer array (CPU)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()
