"""Host references of the fp8 convolution stack's seams (fp8.hip, conv64.hip's e4m3 epilogue): OCP e4m3 rounding two independent ways
(torch's float8_e4m3fn cast, and round-half-even written out in float64), the byte decoding, and the two emulations
tests/test_gpu_fp8_seams.py compares kernels with.  tests/test_fp8_ref.py holds the two roundings to each other on every bf16 pattern,
which is what lets the GPU comparisons be bit-exact statements."""
import numpy as np
import torch

E4M3_MAX = 448.0
FACTORS = (1.0, 1.0 / 3.0, 448.0 / 5.7, 37.0, 1e-3)   # the factors both cast tests run at (as float32)


def _clamped(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).clamp(-E4M3_MAX, E4M3_MAX)


def e4m3(a):
    """round-to-nearest-even OCP e4m3 with saturation at +-448, returned as float32 (torch's float8_e4m3fn cast)."""
    return _clamped(a).to(torch.float8_e4m3fn).to(torch.float32).numpy()


def e4m3_bytes(a):
    """The same rounding, as the e4m3 bytes (uint8 array of a's shape)."""
    return _clamped(a).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def e4m3_rne_numpy(a):
    """Round-half-even to the e4m3 grid in float64, no float8 type involved: clamp to +-448, exponent e = max(floor(log2 |v|), -6)
    (-6: the subnormal binade), grid step 2^(e-3), rint (half to even) of |v| / step.  Finite inputs or infinities; keeps the sign of zero."""
    v = np.clip(np.asarray(a, dtype=np.float64), -E4M3_MAX, E4M3_MAX)
    mag = np.abs(v)
    _, ex = np.frexp(mag)                                  # mag = m * 2^ex with m in [0.5, 1): floor(log2 mag) = ex - 1
    step = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
    return np.copysign(np.rint(mag / step) * step, v).astype(np.float32)


def from_e4m3_bytes(b):
    """e4m3 bytes -> float32 by the format's definition: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent 0 = subnormal
    (m * 2^-9); S.1111.111 = NaN (no infinities)."""
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    ex, m = (b >> 3) & 15, b & 7
    mag = np.where(ex == 0, np.ldexp(m.astype(np.float64), -9), np.ldexp(8.0 + m, ex - 10))
    mag = np.where((ex == 15) & (m == 7), np.nan, mag)
    return np.where(b & 0x80, -mag, mag).astype(np.float32)


def all_bf16_patterns(nan_to_zero=True):
    """Every one of the 65 536 bf16 bit patterns as a bfloat16 tensor in pattern order, NaN patterns replaced by +0."""
    bits = np.arange(65536, dtype=np.int64)
    if nan_to_zero:
        bits = np.where(((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0), 0, bits)
    return torch.as_tensor(bits.astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def scaled(x_bf16, factor):
    """bf16 tensor times the float32 factor, in float32 (overflow to +-inf is meant: it saturates)."""
    with np.errstate(over="ignore"):
        return x_bf16.float().numpy() * np.float32(factor)


def cast_bf16_fp8_ref(x_bf16, factor):
    """cast_bf16_fp8_kernel on the host: the bf16 value times the float32 factor in float32, clamped, rounded half-even -> bytes."""
    return e4m3_bytes(scaled(x_bf16, factor))


def cast_fp8_bf16_ref(b, factor):
    """cast_fp8_bf16_kernel on the host: the decoded byte times the float32 factor in float32, rounded half-even to bf16 -> int16 bits."""
    v = from_e4m3_bytes(b) * np.float32(factor)
    return torch.as_tensor(v).to(torch.bfloat16).view(torch.int16).numpy()


def bf16_round(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(torch.bfloat16).to(dtype)


def conv3x3_relu(x, w, b, dtype=torch.float64):
    """relu(conv3x3(bf16(x), bf16(w)) + b), zero padding, in the reference layouts x (W,H,Cin,N), w (3,3,Cin,Cout) -> (W,H,Cout,N):
    bf16-rounded operands, products summed by torch's CPU conv2d in `dtype` (float64: exact to ~1e-16 relative of the terms)."""
    xt = bf16_round(x, dtype).permute(3, 2, 1, 0).contiguous()      # [n][ci][j][i]
    wt = bf16_round(w, dtype).permute(3, 2, 1, 0).contiguous()      # [co][ci][b][a]
    y = torch.nn.functional.conv2d(xt, wt, torch.as_tensor(b, dtype=dtype), padding=1)
    return y.clamp_(min=0).permute(3, 2, 1, 0).numpy()


# (W, H, Cout, N, wg_cap) of the conv2_1 epilogue test: one tile that is all border; W != H, two channel chunks, tile seams inside an image;
# 11 tiles on 8 / 2 = 4 capped workgroups (the persistent walk goes past one pass of the three-buffer ring); three channel chunks
CONV64_CASES = ((16, 16, 64, 1, 0), (32, 48, 128, 3, 0), (16, 16, 128, 11, 8), (48, 16, 192, 2, 0))


def conv64_case(W, H, Cout, N):
    """Operands of one conv2_1 epilogue case: post-ReLU-like x, He-scaled w, and a bias of the size of the activations with its own value at
    every channel (a bias lost, or applied to another of a chunk's 64 lane positions, cannot hide)."""
    rng = np.random.default_rng(W * 1000 + H * 10 + Cout + N)
    x = np.abs(rng.standard_normal((W, H, 64, N))).astype(np.float32)
    w = (rng.standard_normal((3, 3, 64, Cout)) * np.sqrt(2.0 / (9 * 64))).astype(np.float32)
    b = (rng.standard_normal(Cout) * 20.0).astype(np.float32)
    return x, w, b


def conv64_f8_emulation(acc_relu, inv):
    """conv64.hip's e4m3 epilogue on a host sum: e4m3(min(relu(acc + b) * inv, 448)) with the product formed in float32."""
    return e4m3(np.minimum(np.asarray(acc_relu, dtype=np.float32) * np.float32(inv), np.float32(E4M3_MAX)))
