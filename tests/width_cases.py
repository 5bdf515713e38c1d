"""Width sets shared by tests/test_width_cases.py (CPU) and tests/test_gpu_widths.py (GPU): caption models (E, H1, H2, V) and activity models
(F, H, C) whose widths lie off the multiple-of-4 grid, under 16, above 1024, or differ between the two layers.

The table is the specification; tests/test_width_cases.py asserts the properties each set is there for, so a set cannot quietly lose one.
What a width reaches in csrc/ (ld64(x) = x rounded up to 64):

  H % 4 != 0       prepare_weights_kernel's scalar branches (`vec` false: C = H or E + H is the row length of a parameter's memory image; alA / alB
                   / altA / altB false where a shadow's base is off 4 elements; `cs` = E off the grid), transpose_multi_kernel's vin / vout,
                   the refusing side of decode_epi_on / lstm_epi_on; V % 4 != 0: embed_stage_to_grad_kernel's scalar stores, smax_records_on
  E % 4 != 0       embed_segsum_kernel's `e0 + k < E` tail; with H on the grid (`eodd`) decode_prep_kernel's scalar copy tail and
                   prepare_weights_kernel's permH / giH rows in its scalar branch
  H % 8, 12, 16    the valid-unit count of the last workgroup of lstm_rec_fwd2_kernel<8> / <12>, lstm_rec_bwd_kernel<1, 8> / <2, 12> and the
                   16-unit ring forms
  H < 16           lstm_fused_eligible refuses: bf16 runs GEMM + cell kernel at every batch
  ld64(H) / 64 = 17  launch_lstm_rec_fwd hands over from lstm_rec_fwd2_kernel to the ring forms (R2_KT = 16); launch_lstm_rec_bwd does not
  H <= 64 / > 64   decode_tables_on, smax_records_on

LRCN-1f needs H1 == H2 and the ABI needs an even H2, so the one-layer form of `over1024` takes H = H2 = 1042 (H1 = 1041 is refused by
lrcn_create); `res2` takes H = H1 = 50.
"""
import collections
import functools

import numpy as np

from oracle import oracle as orc


def ld64(x):
    return (x + 63) // 64 * 64


def last_units(H, U):
    """Valid hidden units in the last workgroup of a U-unit recurrence kernel."""
    return H % U or U


# name -> (E, H1, H2, V, n_layers)
CAPTION = {
    "res1": (33, 17, 18, 97, 2),          # H1 % 16 = 1, % 12 = 5, % 8 = 1; h = 9 odd
    "res2": (37, 50, 46, 131, 2),         # H1 % 4 = H2 % 4 = 2, h = 23; E odd: the shadow split cs is off the vector grid
    "res3": (35, 19, 22, 101, 2),         # H1 % 4 = 3, % 8 = 3, % 12 = 7
    "res5": (34, 21, 30, 103, 2),         # H1 % 8 = 5 (the one count of 1..7 the other sets leave out), % 16 = 5, % 12 = 9; H2 % 8 = 6
    "res7": (38, 23, 26, 105, 2),         # H1 % 8 = 7 at a width the fused kernels accept (15 is below their 16), % 12 = 11, % 16 = 7
    "under16": (5, 15, 14, 99, 2),        # no fused step kernels in bf16
    "min": (1, 1, 2, 3, 2),               # the smallest model the ABI accepts
    "over1024": (1037, 1041, 1042, 97, 2),   # 17 K-tiles; ld4H = 66 x 64 for 4164 and 4168 columns; E > 1024; H1 % 8 = 1
    "uneq_a": (64, 200, 72, 301, 2),      # H1 != H2 on nice widths
    "uneq_b": (72, 64, 136, 203, 2),
    "mid_odd": (101, 203, 206, 301, 2),   # H > 64, H % 4 != 0: the routes of 256 rows and more
    "edge64": (64, 64, 64, 301, 2),       # both sides of the H > 64 predicates
    "edge68": (68, 68, 68, 301, 2),
    "eodd": (37, 68, 68, 301, 2),         # E off the vector grid, H on it: the cell-epilogue routes accept, their weight copies split at cs = 37
    "res2_1f": (37, 50, 50, 131, 1),      # LRCN-1f: X1 = E + H / 2 = 62
    "over1024_1f": (1037, 1042, 1042, 97, 1),   # X1 = 1558
}
TWO_LAYER = tuple(n for n, d in CAPTION.items() if d[4] == 2)
FUSED_MIN_H = 16   # lstm_fused_eligible: the step kernels of lstm_fused.hip run from this width

# (F, H, C)
ACTIVITY = ((75, 50, 7), (33, 17, 5), (5, 15, 3), (70, 1041, 11), (1, 1, 2))

# Decode route cases (256 rows and more): name -> (width set, V).  V % 4 = 0, 2, 1.
DECODE_ROUTES = {
    "mid_odd": ("mid_odd", 301),      # decode_epi_on refuses on H % 4 != 0 (and with it tables and records); score records refuse on V % 4
    "mid_odd-v300": ("mid_odd", 300),  # as above for the decode; smax_records_on has no H & 3 term: score records run at H2 % 4 = 2
    "edge64": ("edge64", 300),        # decode_epi_on accepts; tables and records refuse (H = 64)
    "edge68": ("edge68", 300),        # all accept
    "edge68-v302": ("edge68", 302),   # records refuse (V % 4 = 2)
    "edge68-v301": ("edge68", 301),   # records refuse (V % 4 = 1)
    "eodd": ("eodd", 300),            # all accept at E = 37: prepare_weights_kernel's permuted rows (permH) in its scalar branch, the
                                      # gate-interleaved copy (giH) split inside a quad at cs = 37, decode_prep_kernel's tail of 37 % 8 = 5
}
# Decodes under 256 rows: name -> (width set, K)
DECODE_SMALL = {"res1": ("res1", 3), "res2": ("res2", 3), "under16": ("under16", 3), "min": ("min", 2), "over1024": ("over1024", 3)}
NWORD = 8
B_SMALL = 21   # the smallest training batch of the GPU file
Decode = collections.namedtuple("Decode", "name V K N")   # N images of K hypotheses
ROUTE_N, ROUTE_K, SMALL_N = 52, 5, 5                       # 260 rows: past the 256-row threshold with a tail of 4
DECODES = {k: Decode(n, CAPTION[n][3], K, SMALL_N) for k, (n, K) in DECODE_SMALL.items()}
DECODES.update({"route-" + k: Decode(n, V, ROUTE_K, ROUTE_N) for k, (n, V) in DECODE_ROUTES.items()})
# Winner over runner-up of every decode's float64 beam (tests/torch_ref.py): tests/test_gpu_context_reuse.py's margin -- 20 times what nine
# float32 multiplications and a float32 softmax can move a probability by.
TIE_MARGIN = 1.0 + 1e-5


@functools.lru_cache(maxsize=None)
def model(name, V=None):
    """orc.init_weights with the recurrent, projection and output weights doubled (gates away from the linear regime, as
    test_recurrence_kernel_routes_by_batch_size_vs_oracle_bf16), and a bias that matters."""
    E, H1, H2, V0, nl = CAPTION[name]
    V = V or V0
    m = orc.init_weights(E, H1, H2, V, seed=11, n_layers=nl)
    for n in ("W1", "W2", "Wout", "Wproj"):
        if m.p[n].size:
            m.p[n] *= 2.0
    rng = np.random.default_rng(H1 + V)
    m.p["b1"][:] += (rng.standard_normal(m.p["b1"].shape) * 0.5).astype(np.float32)
    return m


class Batch:
    pass


@functools.lru_cache(maxsize=None)
def batch(name, B, T, masks=False):
    """Seeded features, tokens (ids from 0: eos, bos and unk occur as inputs) and, with `masks`, explicit dropout multipliers."""
    E, H1, H2, V, nl = CAPTION[name]
    rng = np.random.default_rng(1000 * B + T)
    c = Batch()
    c.B, c.T = B, T
    c.feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
    c.tokens = rng.integers(0, V, size=(T, B)).astype(np.int32)
    c.mask1 = c.mask2 = None
    if masks:
        c.mask1 = ((rng.random((T + 1, B, E if nl == 2 else E + H2 // 2)) > 0.3) / 0.7).astype(np.float32)
        c.mask2 = ((rng.random((T + 1, B, H2)) > 0.3) / 0.7).astype(np.float32) if nl == 2 else None
    return c


@functools.lru_cache(maxsize=None)
def decode_model(name, V=None):
    """model() with Wout tripled once more and a random output bias: decisive word distributions, as the decode tests' peaked models."""
    E, H1, H2, V0, nl = CAPTION[name]
    V = V or V0
    src = model(name, V)
    m = orc.Model(E, H1, H2, V, {n: a.copy() for n, a in src.p.items()}, nl)
    m.p["Wout"][:] *= 3.0
    m.p["bout"][:] = (np.random.default_rng(V).standard_normal((1, V)) * 2.0).astype(np.float32)
    return m


def decode_feats(N):
    """The decodes' features.  tests/test_width_cases.py asserts that every image's float64 beam then has a winner that leads by TIE_MARGIN
    (the recipe of tests/test_gpu_context_reuse.py; with these decisive models the first seed tried holds for every case)."""
    return (np.random.default_rng(N).standard_normal((N, 4096)) * 0.05).astype(np.float32)


def activity_inputs(F, H, C_, T, B, seed=7):
    """Frame features (B*T) x F, labels and mixed lengths that include 1 and T (B = 1: T)."""
    rng = np.random.default_rng(seed + B)
    x = rng.standard_normal((B * T, F)).astype(np.float32)
    lab = rng.integers(0, C_, B).astype(np.int32)
    lens = rng.integers(1, T + 1, B).astype(np.int32)
    lens[0], lens[-1] = 1, T
    return x, lab, lens


# ---- the unfused update's trajectory (tests/test_gpu_widths.py section d) against orc.adam on the oracle's own gradients
UPDATE_B, UPDATE_T, UPDATE_STEPS = 6, 3, 3
ADAM_SETS = ("res2", "res3", "over1024", "res2_1f")
ADAM_ATOL = 5e-6      # test_adam_trajectory_vs_golden's bound on the parameters
ADAM_LR, ADAM_B2, ADAM_EPS = 1e-3, 0.999, 1e-8
# Elements that adam_reference() finds ill-conditioned, of all the model's elements: measured; tests/test_width_cases.py asserts that the count
# stays within a tenth of these (at most 1 % of any tensor).
ADAM_ILL = {"res2": (143, 141074), "res3": (19, 59263), "over1024": (99380, 20225373), "res2_1f": (72, 136528)}


@functools.lru_cache(maxsize=None)
def update_batches(name):
    V = CAPTION[name][3]
    rng = np.random.default_rng(5)
    return [((rng.standard_normal((UPDATE_B, 4096)) * 0.05).astype(np.float32), rng.integers(0, V, size=(UPDATE_T, UPDATE_B)).astype(np.int32))
            for _ in range(UPDATE_STEPS)]


class AdamRef:
    pass


@functools.lru_cache(maxsize=None)
def adam_reference(name):
    """UPDATE_STEPS steps of orc.adam on the oracle's gradients from model(name): .losses, .params (name -> array), and per tensor .allow, what
    float32 noise in the gradient may add to ADAM_ATOL, .ill, the ill-conditioned elements, and .bound.

    Adam's step is u = m^ / (sqrt(v^) + eps): an element whose gradients are float32 noise (|g| ~ 1e-10 beside a tensor maximum of 4e-3) moves
    by lr in the direction of the noise.  u moves by at most 2 |dg| / (sqrt(v^) + eps) per unit of gradient error and never by more than 2;
    |dg| is MEASURED per step as the difference between the oracle's double-storage gradient on its own trajectory and its float-storage
    gradient on the float-storage trajectory (.float_params) -- the float32 noise of the oracle's own gradient, and from the second step on
    what the noise-driven steps of the ill-conditioned elements feed back into every gradient -- and an element takes the smaller of the
    largest difference in its row and in its column (the noise of a weight gradient scales with its input row and its output column), so
    allow_i = lr sum_t min(2, 2 dg_t,i / (sqrt(v^_t,i) + eps)).  The float build is ONE realisation of float32 noise; sums taken in another
    order may carry several times its differences, so both uses of the allowance give it a factor 5: `ill` is 5 allow > ADAM_ATOL, and .bound,
    what any element may differ by, is ADAM_ATOL + min(5 allow, 2 lr per step)."""
    src = model(name)
    m, mf = (orc.Model(src.E, src.H1, src.H2, src.V, {n: a.copy() for n, a in src.p.items()}, src.n_layers) for _ in range(2))
    names = [n for n in orc.PARAM_NAMES if m.p[n].size]
    mom, momf = ({n: (np.zeros_like(m.p[n]), np.zeros_like(m.p[n])) for n in names} for _ in range(2))
    r = AdamRef()
    r.losses, r.allow = [], {n: np.zeros(m.p[n].shape) for n in names}
    for t, (feats, toks) in enumerate(update_batches(name), 1):
        val, g = orc.loss(m, feats, toks, want_grad=True)
        _, gf = orc.loss(mf, feats, toks, want_grad=True, wide=False)
        r.losses.append(val)
        for n in names:
            orc.adam(m.p[n], g.p[n], mom[n][0], mom[n][1], t)
            orc.adam(mf.p[n], gf.p[n], momf[n][0], momf[n][1], t)
            d = np.abs(g.p[n].astype(np.float64) - gf.p[n])
            dg = np.minimum(d.max(1, keepdims=True), d.max(0, keepdims=True))
            vhat = mom[n][1].astype(np.float64) / (1.0 - ADAM_B2 ** t)
            r.allow[n] += ADAM_LR * np.minimum(2.0, 2.0 * dg / (np.sqrt(vhat) + ADAM_EPS))
    r.float_params = {n: mf.p[n] for n in names}
    r.params = {n: m.p[n] for n in names}
    r.ill = {n: 5 * r.allow[n] > ADAM_ATOL for n in names}
    r.bound = {n: ADAM_ATOL + np.minimum(5 * r.allow[n], 2 * ADAM_LR * UPDATE_STEPS) for n in names}
    return r
