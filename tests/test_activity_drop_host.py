"""CPU: the binding of include/lrcn_act_dropout.h and the dropout references of tests/activity_drop_ref.py themselves (no GPU)."""
import ctypes
import re

import numpy as np

import lrcn_amd
from lrcn_amd import _lib

from activity_drop_ref import emulated_drop, reference_drop, seeded_masks
from activity_ref import emulated, reference


def test_binding_covers_exactly_the_dropout_header():
    lrcn_amd.build()
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.ACT_DROPOUT_HEADER).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(lrcn_act_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["lrcn_act_loss_grad_drop"]
    assert sorted(_lib.ACT_DROPOUT_SIGNATURES) == names
    assert not set(names) & set(_lib.ACTIVITY_SIGNATURES) and not set(names) & set(_lib.SIGNATURES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), "missing export: " + n
    assert '#include "lrcn_activity.h"' in txt
    # lrcn_act_dropout: two floats, the 8-aligned seed, two pointers
    assert ctypes.sizeof(_lib.ActDropout) == 32
    assert [_lib.ActDropout.p_in.offset, _lib.ActDropout.p_out.offset, _lib.ActDropout.seed.offset, _lib.ActDropout.mask_in.offset,
            _lib.ActDropout.mask_out.offset] == [0, 4, 8, 16, 24]


def _tiny(seed=0, F=6, H=4, C=3, T=4, B=3):
    rng = np.random.default_rng(seed)
    W = rng.uniform(-0.5, 0.5, (F + H, 4 * H))
    b = rng.uniform(-0.2, 0.2, (1, 4 * H))
    Wo = rng.uniform(-0.5, 0.5, (H, C))
    bo = rng.uniform(-0.2, 0.2, (1, C))
    x = rng.standard_normal((B * T, F)).astype(np.float32)
    lab = rng.integers(0, C, B)
    lens = np.array([1, T, 2][:B], np.int32)
    return W, b, Wo, bo, x, lab, lens, T, B


def test_hand_written_masked_backward_equals_autograd():
    args = _tiny(F=12, H=8)
    T, B = args[-2:]
    for p_in, p_out in ((0.5, 0.5), (0.9, 0.5), (0.4, 0.0), (0.0, 0.4)):
        mi, mo = seeded_masks(11, p_in, p_out, T, B, 12, 8)
        assert (p_in == 0 or ((mi == 0).any() and (mi > 1).any())) and (p_out == 0 or ((mo == 0).any() and (mo > 1).any()))
        l0, g0 = reference_drop(*args, mi, mo)
        l1, g1 = emulated_drop(*args, mi, mo, bf16=False)
        assert abs(l0 - l1) <= 1e-9 * abs(l0)
        for a, r in zip(g1, g0):
            np.testing.assert_allclose(a, r, rtol=1e-9, atol=1e-9 * np.abs(r).max())
        # the masks matter: the plain model's loss is another one
        assert abs(l0 - reference(*args)[0]) > 1e-3 * abs(l0)


def test_all_ones_masks_are_the_plain_references_exactly():
    args = _tiny(seed=2, F=12, H=8)
    T, B = args[-2:]
    ones = (np.ones((T, B, 12), np.float32), np.ones((T, B, 8), np.float32))
    l0, g0, _, _ = reference(*args)
    for masks in (ones, (None, None)):
        l1, g1 = reference_drop(*args, *masks)
        assert l1 == l0
        for a, r in zip(g1, g0):
            np.testing.assert_array_equal(a, r)
    for bf16 in (False, True):
        l0, g0, _, _ = emulated(*args, bf16=bf16)
        l1, g1 = emulated_drop(*args, *ones, bf16=bf16)
        assert l1 == l0
        for a, r in zip(g1, g0):
            np.testing.assert_array_equal(a, r)


def test_masked_steps_past_a_clips_length_do_not_matter():
    args = _tiny(seed=4, F=12, H=8)
    W, b, Wo, bo, x, lab, lens, T, B = args
    mi, mo = seeded_masks(3, 0.5, 0.5, T, B, 12, 8)
    l0, g0 = reference_drop(*args, mi, mo)
    mi2, mo2 = mi.copy(), mo.copy()
    mi2[1:, 0], mo2[1:, 0] = 7.0, 7.0    # clip 0 has one real frame
    l1, g1 = reference_drop(*args, mi2, mo2)
    assert l1 == l0
    for a, r in zip(g1, g0):
        np.testing.assert_allclose(a, r, rtol=1e-12, atol=1e-15)
