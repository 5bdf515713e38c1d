"""Host restatement of include/lrcn_clip.h (test infrastructure): the sum of squares exactly rounded (math.fsum of float64 squares -- a
float32's square is exact in float64), then lrcn_clip_set's rule word for word, then g * scale as one float32 multiply per element."""
import math

import numpy as np


def sumsq(g):
    """Correctly rounded sum of squares of a float32 array (any shape)."""
    a = np.ascontiguousarray(np.asarray(g, dtype=np.float32)).ravel().astype(np.float64)
    return math.fsum((a * a).tolist())


def clip_from_slots(slots, max_norm):
    """-> (norm: float, scale: np.float32, skip: bool) of lrcn_clip_set over `slots` (added in order, in double)."""
    s = 0.0
    for x in slots:
        s += float(x)
    norm = math.sqrt(s) if s == s else float("nan")
    skip = not math.isfinite(norm)
    mn = float(np.float32(max_norm))
    if not skip and norm > mn:
        scale = np.float32(mn / norm)
    else:
        scale = np.float32(1.0)
    return norm, scale, skip


def scaled(g, scale):
    return np.asarray(g, dtype=np.float32) * np.float32(scale)


def clip(grads, max_norm):
    """grads: list of float32 arrays, one slot each (at most 9) -> (pre-scaled gradients, norm, scale, skip)."""
    assert len(grads) <= 9
    norm, scale, skip = clip_from_slots([sumsq(g) for g in grads], max_norm)
    return [scaled(g, scale) for g in grads], norm, scale, skip
