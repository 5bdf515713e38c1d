"""CPU: the host transcription of the device dropout hash (tests/dropout_ref.py) has the properties a dropout mask must have.  What ties
it to the device is tests/test_gpu_dropout_seeded.py (bit-equal gradients) and tests/test_gpu_embed_grad.py (exported rows are zero exactly
where it drops); here: values, the kept share, independence of streams and seeds, p = 0."""
import numpy as np
import pytest

import dropout_ref as dr

T, B, E, H = 11, 256, 1000, 1000   # the benchmark's step: 3 072 000 elements per mask


@pytest.mark.parametrize("p", [0.4, 0.5])
def test_values_and_kept_share(p):
    m1, m2 = dr.masks(9, p, T, B, E, H)
    mult = dr.multiplier(p)
    assert mult.dtype == np.float32 and mult == np.float32(1) / (np.float32(1) - np.float32(p))
    for m in (m1, m2):
        assert m.dtype == np.float32 and m.shape == (T + 1, B, E)
        n = m.size
        assert n >= 10 ** 6
        kept = int(np.count_nonzero(m))
        assert np.array_equal(np.unique(m), np.array([0, mult], np.float32))
        # u is uniform on multiples of 2^-24 and kept iff u > float32(p): the kept probability is 1 - p to within 2^-24 + |float32(p) - p|
        q = 1.0 - p
        sd = np.sqrt(n * p * q)
        print("p = %.1f: kept %.4f of %d (4 sd = %.4f)" % (p, kept / n, n, 4 * sd / n))
        assert abs(kept - n * q) <= 4 * sd, (kept / n, q)


def test_streams_and_seeds_differ():
    m1, m2 = dr.masks(9, 0.4, T, B, E, H)
    o1, _ = dr.masks(10, 0.4, T, B, E, H)
    # two independent masks at p = 0.4 agree on 0.6^2 + 0.4^2 = 0.52 of the elements
    for a, b in ((m1, m2), (m1, o1)):
        agree = float(np.mean((a != 0) == (b != 0)))
        assert abs(agree - 0.52) < 0.005, agree


def test_p_zero_is_all_ones_and_1f_has_one_mask():
    m1, m2 = dr.masks(3, 0.0, 2, 3, 5, 8)
    assert np.array_equal(m1, np.ones((3, 3, 5), np.float32)) and np.array_equal(m2, np.ones((3, 3, 8), np.float32))
    f1, f2 = dr.masks(3, 0.4, 2, 3, 5, 8, n_layers=1)
    assert f1.shape == (3, 3, 5 + 4) and f2 is None
    # the counter is the C-order index over (s, b, j) with ncols = E + h: not the two-layer stream-1 mask padded
    assert np.array_equal(f1, dr.drop_mult(3, 1, 0.4, 3, 3, 9))


def test_mix64_is_the_splitmix64_finaliser():
    # first outputs of splitmix64 seeded with 0 (state advances by the golden gamma; mix64 adds it itself): public test vectors
    g = 0x9E3779B97F4A7C15
    got = [int(x) for x in dr.mix64(np.array([0, g, (2 * g) & ((1 << 64) - 1)], np.uint64))]
    assert got == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]


def test_the_edge_seed_has_a_uniform_equal_to_p():
    # what makes `u > p` checkable against `u >= p` on the device (tests/test_gpu_dropout_seeded.py, "edge")
    u = dr.hash_uniform(dr.EDGE_SEED, 1, np.arange(6 * 6 * 72, dtype=np.uint64))
    assert u[dr.EDGE_INDEX] == np.float32(dr.EDGE_P) and np.float32(dr.EDGE_P) == dr.EDGE_P
    m1, _ = dr.masks(dr.EDGE_SEED, dr.EDGE_P, 5, 6, 72, 64)
    assert m1.reshape(-1)[dr.EDGE_INDEX] == 0 and dr.multiplier(dr.EDGE_P) == 2
    f1, _ = dr.masks(dr.EDGE_SEED, dr.EDGE_P, 5, 6, 72, 64, n_layers=1)
    assert f1.reshape(-1)[dr.EDGE_INDEX] == 0 and dr.EDGE_INDEX % (72 + 32) < 72   # LRCN-1f: the same counter, an embedding column
    # float32(0.4) is no multiple of 2^-24: no uniform can equal it
    assert (np.float64(np.float32(0.4)) * 2 ** 24) % 1 != 0
