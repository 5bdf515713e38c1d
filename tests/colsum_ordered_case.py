"""The one shape of tests/test_gpu_colsum_ordered.py, shared with its CPU side (tests/test_colsum_ordered_case.py): the bias column sums of a
training step on a context with LRCN_OPT_DETERMINISTIC above 512 rows -- colsum_kernel<T, 64>, one 1024-thread block of 64 row groups per
64 columns, summed in row order -- at a row count that is NO multiple of 64 and widths that fill neither the last column block nor the last
quad:

  B = 48, T = 10     M = (T + 1) B = 528 rows = 8 full passes of the 64 row groups + a tail of 16 rows (row groups 0 .. 15 take a ninth row)
  E = H = 72         b1, b2: 4 H = 288 columns = 4 blocks of 64 + one of 32 (lanes 8 .. 15 of the last block hold no column)
  V = 301            bout: the last quad (columns 300 .. 303 of the padded row) holds one live column

References (nothing from the library): float64 autograd (tests/torch_ref.py) for f32; the bf16-emulating oracle for bf16, in its double- and
its float-accumulating order."""
import functools

import numpy as np
import torch

import torch_ref as tr
from oracle import oracle as orc

E = H = 72
V = 301
B, T = 48, 10
ROWS = (T + 1) * B
BIASES = ("b1", "b2", "bout")


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case():
    c = Case()
    rng = np.random.default_rng(528)
    c.model = orc.init_weights(E, H, H, V, seed=72)
    c.model.p["bout"][:] = (3.0 * rng.standard_normal((1, V))).astype(np.float32)
    for n in ("b1", "b2"):
        c.model.p[n][:] += (0.5 * rng.standard_normal(c.model.p[n].shape)).astype(np.float32)
    c.feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    c.tokens = rng.integers(0, V, size=(T, B)).astype(np.int32)
    c.tokens[0, 0], c.tokens[T - 1, B - 1], c.tokens[3, 17] = V - 1, V - 1, V - 1   # the last quad's one live column is a target, in the
    c.tokens[1, 5] = 256                                                            # tail rows too; so is the last block's first column
    return c


class Result:
    def __init__(self, loss, g):
        self.loss, self.g = float(loss), {n: np.asarray(a, np.float64) for n, a in g.items()}


@functools.lru_cache(maxsize=None)
def reference():
    """float64 autograd: Result (never written to)."""
    c = case()
    p = {n: torch.tensor(c.model.p[n], dtype=torch.float64, requires_grad=True) for n in orc.PARAM_NAMES}
    val = tr.loss(p, torch.tensor(c.feats, dtype=torch.float64), c.tokens, B)
    val.backward()
    return Result(val.item(), {n: p[n].grad.numpy() for n in p})


@functools.lru_cache(maxsize=None)
def emulated(fast=False):
    """(loss, gradient object with .p, and .f32 = the plain f32 oracle's (loss, gradients)) of the bf16-emulating oracle; fast: its
    float-accumulating build -- the same rounding points in another summation order (tests/xent_ladder_cases.py's recipe)."""
    c = case()
    kw = {}
    if fast:
        kw["fast"] = True
        orc.lib(True).orc_set_emulate_bf16(1)
    try:
        with orc.emulate_bf16():
            val, g = orc.loss(c.model, c.feats, c.tokens, norm_B=B, want_grad=True, **kw)
    finally:
        if fast:
            orc.lib(True).orc_set_emulate_bf16(0)
    if not fast:
        g.f32 = orc.loss(c.model, c.feats, c.tokens, norm_B=B, want_grad=True)
    return val, g


def rel_norm(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / (np.linalg.norm(ref) + 1e-300))
