"""Host restatement of the sampled decode's noise (include/lrcn_sample.h, csrc/philox.h): Philox4x32-10 and the Gumbel map, in numpy
uint32 / float32 arithmetic, vectorised over counters."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
PRUNE = 20.0   # GUMBEL_PRUNE: noise is only drawn for columns with z >= max - PRUNE * T (exact: g lies in [-2.812, 16.636])


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counters (broadcastable uint32 arrays) and key words -> the four uint32 output words."""
    c = [np.asarray(x, dtype=np.uint32) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint32(k0), np.uint32(k1)
    mask = np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c[0].astype(np.uint64)
            p1 = M1 * c[2].astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & mask).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & mask).astype(np.uint32)
            c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
            k0 = np.uint32(k0 + W0)
            k1 = np.uint32(k1 + W1)
    return c


def gumbel(x):
    """g = -log(-log(u)), u = ((x >> 9) + 0.5) * 2^-23, all float32."""
    x = np.asarray(x, dtype=np.uint32)
    u = ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    return -np.log(-np.log(u))


def noise(seed, i, s, current, cols):
    """g of columns `cols` for image i, sample s at step `current`."""
    cols = np.asarray(cols, dtype=np.int64)
    w = philox4x32_10((cols >> 2).astype(np.uint32), np.uint32(current), np.uint32(s), np.uint32(i),
                      np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    x = np.choose((cols & 3).astype(np.int64), w)
    return gumbel(x)


def admitted(z, top_k):
    """Columns the draw ranges over: all, or the top_k largest logits (ties at the boundary: lower column)."""
    if top_k == 0:
        return np.arange(z.shape[0])
    order = np.lexsort((np.arange(z.shape[0]), -z))   # z descending, then column ascending
    return np.sort(order[:top_k])


def scores(z, temperature, top_k, seed, i, s, current):
    """(columns, z / T + g) of the admitted columns (T = 0: z itself), float32."""
    z = np.asarray(z, dtype=np.float32)
    cols = admitted(z, top_k)
    if temperature == 0:
        return cols, z[cols]
    T = np.float32(temperature)
    return cols, z[cols] / T + noise(seed, i, s, current, cols)


def draw(z, temperature, top_k, seed, i, s, current):
    cols, sc = scores(z, temperature, top_k, seed, i, s, current)
    return int(cols[np.argmax(sc)])   # argmax returns the first (lowest column) of equal scores


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max()
    return z - (m + np.log(np.exp(z - m).sum()))
