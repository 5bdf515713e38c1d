"""CPU: the activity-recognition binding, clip helpers and the test reference itself (no GPU)."""
import ctypes
import re

import numpy as np

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import activity as A

from activity_ref import emulated, order_task, reference


def test_binding_covers_exactly_the_activity_header():
    lrcn_amd.build()
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.ACTIVITY_HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_act_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(_lib.ACTIVITY_SIGNATURES) == names
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), "missing export: " + n
    # lrcn.h's set is unchanged: none of the new names is in SIGNATURES
    assert not set(names) & set(_lib.SIGNATURES)


def test_param_sizes_and_argument_errors_without_gpu():
    L = _lib.lib()
    s = (ctypes.c_int64 * 4)()
    assert L.lrcn_act_param_sizes(4096, 256, 101, s) == 0
    assert list(s) == [(4096 + 256) * 4 * 256, 4 * 256, 256 * 101, 101]
    for bad in ((0, 8, 3), (8, 0, 3), (8, 8, 0), (-1, 8, 3)):
        assert L.lrcn_act_param_sizes(*bad, s) == -1   # LRCN_EINVAL
    # creation checks its config before touching a device
    h = ctypes.c_void_p()
    for cfg in ((0, 0, 8, 3, 4, 4, 0, 0), (0, 8, 0, 3, 4, 4, 0, 0), (0, 8, 8, 0, 4, 4, 0, 0), (0, 8, 8, 3, 0, 4, 0, 0),
                (0, 8, 8, 3, 4, 0, 0, 0), (0, 8, 8, 3, 4, 4, 2, 0), (0, 8, 8, 5000, 4, 4, 0, 0)):
        assert L.lrcn_act_create(ctypes.byref(_lib.ActConfig(*cfg)), ctypes.byref(h)) == -1, cfg
        assert L.lrcn_act_last_error(None)


def test_clips():
    assert A.clips(40, 16, 8) == [(0, 16), (8, 16), (16, 16), (24, 16)]
    assert A.clips(41, 16, 8) == [(0, 16), (8, 16), (16, 16), (24, 16), (25, 16)]
    assert A.clips(16, 16, 8) == [(0, 16)]
    assert A.clips(5, 16, 8) == [(0, 5)]
    for n in range(1, 60):
        cs = A.clips(n, 16, 8)
        assert all(0 <= s and s + l <= n and 1 <= l <= 16 for s, l in cs)
        assert cs[-1][0] + cs[-1][1] == n   # every frame is covered


def test_gather_clips():
    v = [np.arange(20 * 3, dtype=np.float32).reshape(20, 3), -np.ones((4, 3), np.float32)]
    x, lens = A.gather_clips(v, [(0, 2, 5), (1, 0, 4)], 5)
    assert x.shape == (10, 3) and list(lens) == [5, 4]
    np.testing.assert_array_equal(x[:5], v[0][2:7])
    np.testing.assert_array_equal(x[5:9], v[1])
    np.testing.assert_array_equal(x[9], 0)


def _tiny(seed=0, F=6, H=4, C=3, T=4, B=3):
    rng = np.random.default_rng(seed)
    W = rng.uniform(-0.5, 0.5, (F + H, 4 * H))
    b = rng.uniform(-0.2, 0.2, (1, 4 * H))
    Wo = rng.uniform(-0.5, 0.5, (H, C))
    bo = rng.uniform(-0.2, 0.2, (1, C))
    x = rng.standard_normal((B * T, F))
    lab = rng.integers(0, C, B)
    lens = np.array([1, T, 2][:B], np.int32)
    return W, b, Wo, bo, x, lab, lens, T, B


def test_hand_written_backward_equals_autograd():
    args = _tiny()
    l0, g0, c0, f0 = reference(*args)
    l1, g1, c1, f1 = emulated(*args, bf16=False)
    assert abs(l0 - l1) <= 1e-12 * abs(l0)
    for a, r in zip(g1, g0):
        np.testing.assert_allclose(a, r, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(c1, c0, rtol=1e-12)
    np.testing.assert_allclose(f1, f0, rtol=1e-12)
    np.testing.assert_allclose(c0.sum(0), 1.0, rtol=1e-12)
    # masked steps: zero frame probabilities, and they do not move the loss
    W, b, Wo, bo, x, lab, lens, T, B = args
    assert np.all(f0[:, 0 * T + 1:0 * T + T] == 0)
    x2 = x.copy()
    x2[0 * T + 1:0 * T + T] += 5.0
    l2, g2, c2, _ = reference(W, b, Wo, bo, x2, lab, lens, T, B)
    assert abs(l2 - l0) <= 1e-12 and np.allclose(c2, c0, rtol=1e-12)
    for a, r in zip(g2, g0):
        np.testing.assert_allclose(a, r, rtol=1e-10, atol=1e-14)


def test_bf16_emulation_stays_near_f64():
    args = _tiny(seed=3, F=32, H=16, C=5, T=6, B=3)
    l0, g0, _, _ = reference(*args)
    l1, g1, _, _ = emulated(*args, bf16=True)
    assert abs(l1 - l0) <= 2e-2 * abs(l0)
    for a, r in zip(g1, g0):
        assert np.linalg.norm(a - r) <= 5e-2 * np.linalg.norm(r)


def test_order_task_is_not_solvable_per_frame():
    x, lab = order_task(64, 8, 16, seed=1)
    assert x.shape == (64 * 8, 16) and set(np.unique(lab)) <= {0, 1}
    # the multiset of frames' pattern content is the same for both classes: per-clip frame means do not separate them
    m = x.reshape(64, 8, 16).mean(1)
    d = m[lab == 0].mean(0) - m[lab == 1].mean(0)
    assert np.abs(d).max() < 0.2
