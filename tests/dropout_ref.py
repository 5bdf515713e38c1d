"""Host transcription of the device-generated dropout mask (tests only; numpy, no GPU, nothing of the code under test).

csrc/kernel_util.h: element (s, b, j) of a (T+1) x [B x ncols] tensor has the counter idx = (s B + b) ncols + j; its uniform is
hash_uniform(seed, which, idx) = float(mix64(mix64(seed ^ which * K) ^ idx) >> 40) * 2^-24 (mix64: the splitmix64 finaliser), and drop_mult
keeps it iff u > p, with the multiplier 1 / (1 - p), everything in float32.  Here: uint64 arrays (numpy wraps them silently), float32 for u, p
and the multiplier, `u > float32(p)`, `float32(1) / (float32(1) - float32(p))`.  The top 24 bits of a hash convert to float32 exactly and
2^-24 is a power of two, so u is exact and the only rounding of the whole transcription is the one division.

The route code of train.hip never looks at a mask (make_drop is the only reader), so a call with (pdrop, seed) and a call with these
arrays as explicit masks are the same arithmetic: tests/test_gpu_dropout_seeded.py demands bit-equal results.
"""
import numpy as np

U64 = np.uint64
_MASK64 = (1 << 64) - 1
_GOLDEN, _M1, _M2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)
_STREAM = 0xD1342543DE82EF95


def mix64(z):
    """mix64 of kernel_util.h on a uint64 array (wrapping)."""
    z = np.asarray(z, U64) + _GOLDEN
    z = (z ^ (z >> U64(30))) * _M1
    z = (z ^ (z >> U64(27))) * _M2
    return z ^ (z >> U64(31))


def hash_uniform(seed, stream, idx):
    """hash_uniform of kernel_util.h: float32 uniforms in [0, 1) for a uint64 array of counters."""
    key = (int(seed) & _MASK64) ^ ((int(stream) * _STREAM) & _MASK64)
    h = mix64(mix64(np.array([key], U64)) ^ np.asarray(idx, U64))
    return (h >> U64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def multiplier(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def drop_mult(seed, which, p, S, B, ncols):
    """drop_mult of kernel_util.h for every element of one tensor: float32 (S, B, ncols), the counter being the C-order index."""
    if np.float32(p) <= 0:
        return np.ones((S, B, ncols), np.float32)
    u = hash_uniform(seed, which, np.arange(S * B * ncols, dtype=U64))
    return np.where(u > np.float32(p), multiplier(p), np.float32(0)).astype(np.float32).reshape(S, B, ncols)


def masks(seed, p, T, B, E, H2, n_layers=2):
    """(mask1, mask2) in the logical (T+1, B, ncols) layout L.lossgradient takes.  Two layers: stream 1 over the E embedding columns
    (lrcn.jl:542), stream 2 over the H2 columns of hcat(projection, x_cnn) (:547).  LRCN-1f: stream 1 over the E + H2/2 columns of
    hcat(embedding, x_cnn), and no second mask."""
    if n_layers == 1:
        return drop_mult(seed, 1, p, T + 1, B, E + H2 // 2), None
    return drop_mult(seed, 1, p, T + 1, B, E), drop_mult(seed, 2, p, T + 1, B, H2)


# An input on which `u > p` and `u >= p` differ: at this seed the stream-1 uniform of counter EDGE_INDEX is exactly 0.5 (found by search over
# seeds; the chance is 2^-24 per element).  The counter lies inside the first mask of any tensor of more than EDGE_INDEX elements.
EDGE_SEED, EDGE_P, EDGE_INDEX = 5206, 0.5, 1697
