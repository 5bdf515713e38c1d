"""CPU: tests/smooth_ref.py, the float64 reference of label smoothing (include/lrcn_smooth.h), against what it restates: torch's
cross_entropy(label_smoothing=) and its autograd on rows, tests/sched_ref.py's loss at eps = 0 on the model, and finite differences."""
import numpy as np
import pytest
import torch

import sched_ref as sr
import smooth_ref as smr
from oracle import oracle as orc


@pytest.mark.parametrize("V", [97, 2049, 16385])
@pytest.mark.parametrize("eps", [0.1, 1.0, 0.0])
def test_rows_equal_torch_cross_entropy_and_its_autograd(V, eps):
    rng = np.random.default_rng(V)
    M = 5
    z = rng.standard_normal((M, V)) * 3.0
    z[1, 7] = 100.0
    tgt = rng.integers(0, V, size=M)
    tgt[1] = 7 if eps == 1.0 else 11
    terms, ll, dlog = smr.xent_rows(z, tgt, eps, scale=1.0)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    ce = torch.nn.functional.cross_entropy(zt, torch.as_tensor(tgt), reduction="none", label_smoothing=eps)
    ce.sum().backward()
    np.testing.assert_allclose(-terms, ce.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dlog, zt.grad.numpy(), rtol=0, atol=1e-12)
    plain = torch.nn.functional.cross_entropy(zt.detach(), torch.as_tensor(tgt), reduction="none")
    np.testing.assert_allclose(-ll, plain.numpy(), rtol=1e-12, atol=1e-12)
    assert np.abs(dlog.sum(1)).max() <= 1e-12


def test_rows_weights_scale_and_inactive_rows():
    rng = np.random.default_rng(5)
    M, B, V = 6, 3, 17
    z = rng.standard_normal((M, V)) * 3.0
    tgt = rng.integers(0, V, size=M)
    tgt[4] = -1
    z[4] = np.nan
    w = np.array([0.0, -1.5, 2.0], np.float32)   # caption 0 (rows 0 and 3) has weight 0
    z[3] = np.nan
    terms, ll, dlog = smr.xent_rows(z, tgt, 0.1, row_w=w, B=B, scale=0.25)
    one_t, one_ll, one_d = smr.xent_rows(np.nan_to_num(z), np.abs(tgt), 0.1, scale=1.0)
    for m in range(M):
        if m in (0, 3, 4):
            assert terms[m] == 0.0 and ll[m] == 0.0 and not dlog[m].any()
        else:
            np.testing.assert_allclose(terms[m], float(w[m % B]) * one_t[m], rtol=1e-14)
            np.testing.assert_allclose(ll[m], float(w[m % B]) * one_ll[m], rtol=1e-14)
            np.testing.assert_allclose(dlog[m], 0.25 * float(w[m % B]) * one_d[m], rtol=1e-14, atol=1e-18)


def _tiny(n_layers):
    B, T, E, H, V = 3, 2, 8, 8, 17
    rng = np.random.default_rng(40 + n_layers)
    m = orc.init_weights(E, H, H, V, seed=3, n_layers=n_layers)
    feats = (rng.standard_normal((B, 4096)) * 0.02).astype(np.float32)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    lens = np.array([2, 0, 1], np.int32)
    w = np.array([1.25, -0.5, 2.0], np.float32)
    return m, feats, tokens, lens, w


@pytest.mark.parametrize("n_layers", [2, 1])
def test_eps_zero_is_the_sched_reference(n_layers):
    m, feats, tokens, lens, w = _tiny(n_layers)
    fed = sr.gold_inputs(tokens, lens)
    fed[1, 0] = 5   # a fed word that is not the gold one
    for row_w in (None, w):
        ref, ref_g = sr.loss(m, feats, tokens, lens, fed, norm_tokens=11, row_w=row_w, want_grad=True)
        val, nll, g = smr.loss(m, feats, tokens, lens, 0.0, fed=fed, norm_tokens=11, row_w=row_w, want_grad=True)
        assert val == ref and nll == ref
        for n in orc.PARAM_NAMES:
            assert np.array_equal(g.p[n], ref_g.p[n]), n
    # eps > 0: the plain sum it reports beside the smoothed loss is still that reference's
    val, nll = smr.loss(m, feats, tokens, lens, 0.1, fed=fed, norm_tokens=11, row_w=w)
    assert abs(nll - sr.loss(m, feats, tokens, lens, fed, norm_tokens=11, row_w=w)) <= 1e-14 and val != nll


@pytest.mark.parametrize("n_layers", [2, 1])
def test_one_gradient_element_per_tensor_against_finite_differences(n_layers):
    m, feats, tokens, lens, w = _tiny(n_layers)
    eps = 0.1
    _, _, g = smr.loss(m, feats, tokens, lens, eps, row_w=w, want_grad=True)
    rng = np.random.default_rng(9)
    h = 1e-6
    for n in orc.PARAM_NAMES:
        a = np.asarray(m.p[n])
        if not a.size:
            continue
        # an element whose gradient is not 0: Wembed's rows of words that are never fed have none
        nz = np.argwhere(np.abs(g.p[n]) > 1e-9)
        idx = tuple(nz[rng.integers(len(nz))])
        old = a[idx]
        vals = []
        for sign in (1.0, -1.0):
            m.p[n] = np.array(a, dtype=np.float64)
            m.p[n][idx] = float(old) + sign * h
            vals.append(smr.loss(m, feats, tokens, lens, eps, row_w=w)[0])
        m.p[n] = a
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - g.p[n][idx]) <= 1e-6 * max(1.0, abs(fd)), (n, idx, fd, g.p[n][idx])
