"""The training softmax ladder's cases, shared by tests/test_xent_ladder_cases.py (CPU) and tests/test_gpu_xent_ladder.py (GPU).

launch_softmax_xent (csrc/xent.hip) picks softmax_xent_reg_kernel<T, Q, FORM> with Q = 2, 4, 8, 12, 16 for V <= 2048, 4096,
8192, 12288, 16384 and the streaming softmax_xent_kernel above.  VOCABS holds the last V of every rung, the first of the next, and a V that
is no multiple of 4 inside the two widest rungs.  A thread's q-th load of the register kernel covers columns 1024 q + 4 tid .. + 3, so the
columns where a rung can go wrong are critical_columns(V): the first and last thread of the first two slots, both sides of the rung's last
slot, and the last four columns (the partial 16-byte load / store).

The model is the smallest that runs (E = H = 16, two layers, B = 5, T = 2: 15 logit rows) from orc.init_weights, with Wout at its initial
scale -- the logits are then bout plus ~1e-2, the sharpness does not pass through bf16 h and the elementwise emulation check stays
meaningful -- and bout ~ N(0, 3^2) plus 4 on the critical columns.  Targets are critical columns only.  With that bout a critical column's
softmax mass is ~1e-4 .. 1e-5 at these widths (16384 columns of mean exp(4.5)), so what makes |g_bout| large on a critical column is being
a TARGET: token_table() hands the columns out by priority -- the rung's last slot and the last four columns first -- to the rows that stay
active in every form, then to the others.  The equal-length form covers every critical column; the masked forms have 6 and 5 active token
targets for up to 8 columns and cover the high-priority ones (asserted on the CPU).

Three forms: `equal` (norm_B = B), `lens` (LENS, a row of length 0 and rows that end early) and `weighted` (LENS and WEIGHTS, a zero-weight
row with active steps).  NORM_TOKENS = 12 makes every row's norm_tokens / (|w| (len + 1)) an integer, so the emulating oracle rounds
d(logits) at the library's scale (tests/varlen_ref.py, tests/weighted_ref.py).  `hot` (V = 16384 and 16385): the equal form with one logit
of ~+100, which overflows float32 exp without the max-subtraction.

References: f32 -- float64: torch autograd (tests/torch_ref.py) for `equal`, `lens` and `hot`, the per-row float64 combination of the
oracle (tests/weighted_ref.py) for `weighted`.  bf16 -- the bf16-emulating oracle, in its two accumulation orders.
"""
import functools

import numpy as np
import torch

import torch_ref as tr
import varlen_ref as vr
import weighted_ref as wr
from oracle import oracle as orc

VOCABS = (2048, 2049, 4096, 4097, 8190, 8192, 8193, 12288, 12289, 16383, 16384, 16385)
HOT_VOCABS = (16384, 16385)
FORMS = ("equal", "lens", "weighted")
E = H = 16
B, T = 5, 2
LENS = np.array((2, 0, 1, 2, 1), np.int32)
WEIGHTS = np.array((1.0, 0.5, 0.0, 2.0, 1.0), np.float32)
NORM_TOKENS = 12
HOT_LOGIT = 100.0
F32_ATOL = 1e-5            # the elementwise atol of the f32 gradient check
FLT_EXP_MAX = 88.72        # float32 exp overflows above


def rung(V):
    """Q of the register kernel that launch_softmax_xent picks, or None for the streaming kernel."""
    for q in (2, 4, 8, 12, 16):
        if V <= 1024 * q:
            return q
    return None


def critical_columns(V):
    """By priority: the rung's last slot's first column, the last four columns, the column below the last slot, the first two slots' seam,
    column 0 (eos: every row's final target).  Above 16384 (no rung) the slot a 17th load would have."""
    q = rung(V) or -(-V // 1024)
    out = []
    for c in (1024 * (q - 1), V - 1, V - 2, V - 3, V - 4, 1024 * (q - 1) - 1, 1024, 1023, 0):
        if 0 <= c < V and c not in out:
            out.append(c)
    return out


def token_table(V):
    """tokens [T][B]: the critical columns other than 0 in priority order, first to the (t, b) that are active in the weighted form, then to the
    one the lens form adds, then to the rest (cycling)."""
    cols = [c for c in critical_columns(V) if c != 0]
    active_w = [(t, b) for b in range(B) for t in range(T) if t < LENS[b] and WEIGHTS[b] != 0]
    active_l = [(t, b) for b in range(B) for t in range(T) if t < LENS[b] and WEIGHTS[b] == 0]
    rest = [(t, b) for b in range(B) for t in range(T) if t >= LENS[b]]
    tok = np.zeros((T, B), np.int32)
    for i, (t, b) in enumerate(active_w + active_l + rest):
        tok[t, b] = cols[i % len(cols)]
    return tok


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(V, hot=False):
    c = Case()
    c.V, c.hot = V, hot
    rng = np.random.default_rng(7000 + V)
    c.model = orc.init_weights(E, H, H, V, seed=V)
    c.crit = critical_columns(V)
    bout = 3.0 * rng.standard_normal((1, V))
    bout[0, c.crit] += 4.0
    if hot:
        c.hot_col = c.crit[0]
        bout[0, c.hot_col] = HOT_LOGIT
    c.model.p["bout"][:] = bout.astype(np.float32)
    c.feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    c.tokens = token_table(V)
    return c


def form_kwargs(form):
    """What L.lossgradient takes beside (ctx, param, feats, tokens)."""
    if form == "equal":
        return dict(norm_B=B)
    kw = dict(lens=LENS, norm_tokens=NORM_TOKENS)
    if form == "weighted":
        kw["row_weights"] = WEIGHTS
    return kw


class Result:
    def __init__(self, loss, g):
        self.loss, self.g = float(loss), {n: np.asarray(a, np.float64) for n, a in g.items()}


def _torch_params(model, requires_grad):
    return {n: torch.tensor(model.p[n], dtype=torch.float64, requires_grad=requires_grad) for n in orc.PARAM_NAMES}


@functools.lru_cache(maxsize=None)
def reference(V, form, hot=False):
    """float64: Result with .logits ((T + 1, B, V), the equal and lens forms)."""
    c = case(V, hot)
    if form == "weighted":
        val, g = wr.loss(c.model, c.feats, c.tokens, LENS, WEIGHTS, NORM_TOKENS, want_grad=True)
        return Result(val, g.p)
    p = _torch_params(c.model, True)
    logits = []
    kw = dict(lens=LENS, norm_tokens=NORM_TOKENS) if form == "lens" else {}
    val = tr.loss(p, torch.tensor(c.feats, dtype=torch.float64), c.tokens, B, collect=logits, **kw)
    val.backward()
    r = Result(val.item(), {n: p[n].grad.numpy() for n in p})
    r.logits = np.stack([y.numpy() for y in logits])
    return r


@functools.lru_cache(maxsize=None)
def emulated(V, form, fast=False):
    """(loss, gradient object with .p and .f32) of the bf16-emulating oracle; fast: its float-accumulating build -- the same rounding points
    in another summation order."""
    c = case(V)
    kw = {}
    if fast:
        kw["fast"] = True
        orc.lib(True).orc_set_emulate_bf16(1)
    try:
        with orc.emulate_bf16():
            if form == "equal":
                val, g = orc.loss(c.model, c.feats, c.tokens, norm_B=B, want_grad=True, **kw)
            elif form == "lens":
                val, g = vr.loss(c.model, c.feats, c.tokens, LENS, NORM_TOKENS, want_grad=True, row_norms=vr.integer_row_norms(LENS, NORM_TOKENS), **kw)
            else:
                val, g = wr.loss(c.model, c.feats, c.tokens, LENS, WEIGHTS, NORM_TOKENS, want_grad=True,
                                 row_norms=wr.integer_row_norms(LENS, WEIGHTS, NORM_TOKENS), **kw)
    finally:
        if fast:
            orc.lib(True).orc_set_emulate_bf16(0)
    if not fast:   # the plain f32 oracle beside it: parity_util's second, independent bound
        if form == "equal":
            g.f32 = orc.loss(c.model, c.feats, c.tokens, norm_B=B, want_grad=True)
        elif form == "lens":
            g.f32 = vr.loss(c.model, c.feats, c.tokens, LENS, NORM_TOKENS, want_grad=True)
        else:
            g.f32 = wr.loss(c.model, c.feats, c.tokens, LENS, WEIGHTS, NORM_TOKENS, want_grad=True)
    return val, g


def rel_norm(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / (np.linalg.norm(ref) + 1e-300))
