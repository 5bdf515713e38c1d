"""CPU: tests/weighted_ref.py, the reference of the weighted caption loss (include/lrcn_weighted.h), against tests/varlen_ref.py, its own
linearity, finite differences of the plain oracle and row omission.  No GPU, no HIP library."""
import numpy as np
import pytest

from oracle import oracle as orc

import varlen_ref as vr
import weighted_ref as wr


def case(seed, B=5, T=4, E=8, H=8, V=11, n_layers=2):
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed + 1, n_layers=n_layers)
    feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    tokens = rng.integers(0, V, size=(T, B)).astype(np.int32)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    return rng, m, feats, tokens, lens


@pytest.mark.parametrize("n_layers", [2, 1])
def test_weights_of_one_are_varlen_ref_exactly(n_layers):
    rng, m, feats, tokens, lens = case(3, n_layers=n_layers)
    for nt in (None, 3 * vr.norm_tokens_of(lens)):
        a, ga = vr.loss(m, feats, tokens, lens, nt, want_grad=True)
        b, gb = wr.loss(m, feats, tokens, lens, np.ones(len(lens), np.float32), nt, want_grad=True)
        assert a == b and wr.loss(m, feats, tokens, lens, np.ones(len(lens)), nt) == a
        for n in orc.PARAM_NAMES:
            assert np.array_equal(ga.p[n], gb.p[n]), n


def test_the_reference_is_linear_in_the_weights():
    rng, m, feats, tokens, lens = case(4)
    w1 = (rng.integers(-16, 17, size=len(lens)) / 8).astype(np.float32)   # eighths: w1 + w2 is exact in float32
    w2 = (rng.integers(-16, 17, size=len(lens)) / 8).astype(np.float32)
    w2[2] = -w1[2]    # a row whose weights cancel: left out of the sum
    ws = w1 + w2
    assert ws[2] == 0 and np.abs(ws).max() > 0
    (a, ga), (b, gb), (s, gs) = (wr.loss(m, feats, tokens, lens, w, want_grad=True) for w in (w1, w2, ws))
    assert abs(s - (a + b)) <= 1e-12 * (abs(a) + abs(b))
    for n in orc.PARAM_NAMES:
        np.testing.assert_allclose(gs.p[n], ga.p[n] + gb.p[n], rtol=0, atol=1e-12 * max(1.0, np.abs(ga.p[n]).max() + np.abs(gb.p[n]).max()), err_msg=n)


def plain_weighted_loss(m, feats, tokens, lens, w, nt):
    """The formula written out on the plain oracle's one-row values: orc.loss of row b is -(1 / (len_b + 1)) sum_s log p."""
    return sum(float(w[b]) * (int(lens[b]) + 1) / nt * orc.loss(m, feats[b:b + 1], tokens[:int(lens[b]), b:b + 1], norm_B=1) for b in range(len(lens)))


def test_finite_differences_of_the_plain_oracles_weighted_loss():
    # eps and the bound of tests/test_oracle_golden.py: test_finite_difference_gradient
    rng = np.random.default_rng(0)
    B, T, E, H, V = 3, 2, 8, 8, 11
    m = orc.init_weights(E, H, H, V, seed=7)
    feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    tokens = rng.integers(0, V, size=(T, B)).astype(np.int32)
    lens = np.asarray([2, 0, 1], np.int32)
    w = np.asarray([1.5, -0.75, 0.5], np.float32)
    nt = 11
    val, g = wr.loss(m, feats, tokens, lens, w, nt, want_grad=True)
    assert abs(val - plain_weighted_loss(m, feats, tokens, lens, w, nt)) <= 1e-12 * abs(val)
    for n in orc.PARAM_NAMES:
        a = m.p[n]
        i, j = np.unravel_index(int(rng.integers(a.size)), a.shape, order="F")
        old, eps = a[i, j], 2e-2
        a[i, j] = old + eps
        lp = plain_weighted_loss(m, feats, tokens, lens, w, nt)
        a[i, j] = old - eps
        lm = plain_weighted_loss(m, feats, tokens, lens, w, nt)
        a[i, j] = old
        fd = (lp - lm) / (2 * eps)
        assert abs(fd - g.p[n][i, j]) <= 3e-3 * max(1e-3, abs(fd)) + 2e-5, (n, i, j, fd, g.p[n][i, j])


def test_a_zero_weight_row_is_the_row_left_out_with_norm_tokens_kept():
    rng, m, feats, tokens, lens = case(6)
    w = rng.standard_normal(len(lens)).astype(np.float32)
    w[[1, 3]] = 0.0
    nt = vr.norm_tokens_of(lens)
    a, ga = wr.loss(m, feats, tokens, lens, w, nt, want_grad=True)
    keep = [0, 2, 4]
    b, gb = wr.loss(m, feats[keep], tokens[:, keep], lens[keep], w[keep], nt, want_grad=True)
    assert a == b
    for n in orc.PARAM_NAMES:
        assert np.array_equal(ga.p[n], gb.p[n]), n
    other = tokens.copy()
    other[:, [1, 3]] = (other[:, [1, 3]] + 1) % 11     # a zero-weight row's tokens are never looked at
    assert wr.loss(m, feats, other, lens, w, nt) == a


@pytest.mark.parametrize("B", [256, 48])
def test_the_bf16_cases_of_the_gpu_test_have_integer_row_norms(B):
    # the seeds tests/test_gpu_weighted.py uses: every n_b = norm_tokens / (|w_b| (len_b + 1)) is an integer (bf16_case asserts it)
    lens, w, nt = wr.bf16_case(B, np.random.default_rng(B))
    nb = wr.integer_row_norms(lens, w, nt)
    assert nt == 4 * vr.norm_tokens_of(lens) and set(np.abs(w).tolist()) <= {0.5, 1.0, 2.0} and (w < 0).any() and (w > 0).any()
    for n, x, q in zip(lens, w, nb):
        assert q * abs(float(x)) * (int(n) + 1) == nt
    assert lens.max() <= 5
