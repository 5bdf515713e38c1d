"""CPU: the host restatement of gradient-norm clipping (tests/clip_ref.py) on hand cases."""
import math

import numpy as np

import clip_ref


def test_norm_below_equal_and_above_max_norm():
    g = [np.array([3.0, 0.0], np.float32), np.array([[4.0]], np.float32)]   # norm exactly 5
    for max_norm, want in ((6.0, 1.0), (5.0, 1.0), (2.5, 0.5)):
        out, norm, scale, skip = clip_ref.clip(g, max_norm)
        assert norm == 5.0 and not skip
        assert scale.dtype == np.float32 and scale == np.float32(want)
        assert all(o.dtype == np.float32 for o in out)
        np.testing.assert_array_equal(out[0], np.array([3.0 * want, 0.0], np.float32))
        np.testing.assert_array_equal(out[1], np.array([[4.0 * want]], np.float32))
    # the quotient is taken in double and rounded to float once
    _, norm, scale, _ = clip_ref.clip([np.array([1.0, 1.0, 1.0], np.float32)], 1.0)
    assert norm == math.sqrt(3.0) and scale == np.float32(1.0 / math.sqrt(3.0))


def test_inf_and_nan_give_skip():
    for bad in (np.inf, -np.inf, np.nan):
        g = [np.array([1.0, bad, 2.0], np.float32), np.ones(4, np.float32)]
        out, norm, scale, skip = clip_ref.clip(g, 1.0)
        assert skip and not math.isfinite(norm) and scale == np.float32(1.0)
    # a non-finite slot anywhere
    assert clip_ref.clip_from_slots([1.0, float("inf"), 2.0], 5.0)[2]
    assert clip_ref.clip_from_slots([float("nan")], 5.0)[2]


def test_squares_that_overflow_float_stay_finite():
    g = [np.full(1000, 1e30, np.float32)]
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(1e30) * np.float32(1e30))
    out, norm, scale, skip = clip_ref.clip(g, 5.0)
    assert not skip and math.isfinite(norm)
    x = float(np.float32(1e30))
    assert norm == math.sqrt(math.fsum([x * x] * 1000))
    assert scale == np.float32(5.0 / norm) and np.all(np.isfinite(out[0]))


def test_sum_is_exactly_rounded_and_slot_order_is_kept():
    rng = np.random.default_rng(0)
    a = (rng.standard_normal(5000) * 10.0 ** rng.uniform(-12, 12, 5000)).astype(np.float32)
    from fractions import Fraction
    exact = sum(Fraction(float(x)) ** 2 for x in a)
    assert clip_ref.sumsq(a) == float(exact)
    assert clip_ref.sumsq(np.zeros(0, np.float32)) == 0.0
    # slots are added in order, in double: (1 + 2^-53) + 2^-53 rounds to 1 twice, 2^-53 + 2^-53 + 1 does not
    t = 2.0 ** -53
    assert clip_ref.clip_from_slots([1.0, t, t], 10.0)[0] == 1.0
    assert clip_ref.clip_from_slots([t, t, 1.0], 10.0)[0] == math.sqrt(1.0 + 2.0 ** -52)
