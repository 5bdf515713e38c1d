"""Production-width cases shared by tests/test_oracle_production_width.py (CPU) and tests/test_gpu_production_width.py (GPU).

Each case is a batch at the caption model's real widths (E = H = 512 / V = 2540 of BASELINE config 1, E = H = 1000 / V = 10640 of config 4)
in two regimes, and its reference is the float64 autograd transcription of tests/torch_ref.py, computed at test time, once per process:

  init   orc.init_weights as it stands and random targets: logits of ~1e-2, a uniform softmax, gates in the linear part of sigmoid / tanh.
  sharp  sharpen() below: a trained-like model.  W1, W2 x 4 and Wcnn x 12, Wembed rescaled to rms 1.3, Wout rescaled to the first rung of
         SHARP_WOUT_RMS (rms 1 .. 6; xavier's is 0.026) at which the case reaches mean p(target) >= 0.4, bout ~ N(0, 1), b1 / b2 + N(0, 0.5);
         the targets are the transcription's own greedy decode (ids below 3 lifted to 3) with random ids swapped in until, with each row's
         final eos, 15 % of the loss terms are ones the model does not predict.  (The milder recipe first tried -- W1, W2 x 4, Wout x 64
         only -- saturates 0.01 % of the gates, not 10 %: the embedding and the image input have to grow too.)  softmax - onehot then
         cancels on most rows, the max-subtraction matters and a good share of the gates saturate.  Measured: max |logit| 32 .. 51 in the CPU
         cases (Wout rms 1 .. 1.5), 45 in c1-rows256 and 121 in c4-rows64 (T = 1, rms 4: float32 exp overflows there without the
         max-subtraction).  c4-rows64's loss is 56.6: with T = 1 half of its loss terms are the final eos, which this model never predicts and
         which costs ~110 nats at such logits; the other half it predicts.  reference() ASSERTS the regime from the float64 numbers alone
         (mean p(target) >= 0.4 over the active loss terms, >= 10 % of layer 1's gate pre-activations beyond |z| = 3, every logit
         finite), so a case cannot quietly fall back to the flat regime.

The oracle (oracle/lrcn_oracle.c) enters only through oracle_result(), as the thing under test (CPU file) or as the bf16 emulation floor.
"""
import functools
import json
import os

import numpy as np
import torch

import dropout_ref as dr
import torch_ref as tr
import varlen_ref as vr
from oracle import oracle as orc

REGIMES = ("init", "sharp")
C1 = dict(E=512, V=2540)
C4 = dict(E=1000, V=10640)
CASES = {
    "c1": dict(C1, B=16, T=11),                              # fused small-batch recurrence, skinny GEMMs
    "c4-slice": dict(C4, B=8, T=3),                          # H = 1000 tails, V = 10640 softmax
    "c1-masks": dict(C1, B=16, T=5, keep=0.6, norm_B=64),    # explicit dropout masks, a global batch of 4 B
    "c1-seeded": dict(C1, B=16, T=5, pdrop=0.4, seed=0xC0FFEE0000000123, norm_B=64),   # c1-masks' shape, the DEVICE-generated masks
    "1f": dict(C1, B=16, T=5, n_layers=1),                   # LRCN-1f
    "varlen": dict(C1, B=13, T=7, lens=(7, 0, 3, 1, 7, 3, 0, 1, 3, 7, 1, 3, 7)),   # sum(lens + 1) = 56, a multiple of every len + 1
    "c1-rows256": dict(C1, B=256, T=3),                      # GEMM + cell kernel, >= 256-row xent and embedding scatter
    "c4-rows64": dict(C4, B=64, T=1),                        # the 64-row boundary of the fused forms
}
CPU_CASES = ("c1", "c4-slice", "c1-masks", "1f", "varlen", "c1-seeded")
GPU_CASES = ("c1", "c1-rows256", "c4-slice", "c4-rows64", "1f", "varlen", "c1-seeded")
# A case's inputs are seeded by its number.  Cases added after the first seven take the next numbers, so that the earlier ones keep theirs.
_LATER = ("c1-seeded",)
CASE_NUMBER = {n: i for i, n in enumerate(sorted(set(CASES) - set(_LATER)) + list(_LATER))}
SHARP_SCALE = {"W1": 4.0, "W2": 4.0, "Wcnn": 12.0}
SHARP_RMS = {"Wembed": 1.3}
SHARP_WOUT_RMS = (1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 6.0)   # rungs of Wout's rms: a case takes the first at which mean p(target) reaches P_TARGET_MIN
P_TARGET_MIN, SATURATED_MIN = 0.4, 0.10
SHARP_MISSES = 0.15   # share of the loss terms whose target the model does not predict: each row's final eos, plus random replacements
DIGEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "production_width_digest.json")


class Case:
    pass


def live(model):
    return [n for n in orc.PARAM_NAMES if model.p[n].size]


def torch_params(model, dtype=torch.float64, requires_grad=False):
    return {n: torch.tensor(model.p[n], dtype=dtype, requires_grad=requires_grad) for n in live(model)}


def _t(a, dtype):
    return None if a is None else torch.tensor(a, dtype=dtype)


def transcription_loss(c, p, dtype=torch.float64, **kw):
    """The transcription's loss of case c with parameters p (a torch scalar)."""
    if c.lens is not None:
        kw.update(lens=c.lens, norm_tokens=c.norm_tokens)
    if c.n_layers == 1:
        return tr.loss1(p, _t(c.feats, dtype), c.tokens, c.norm_B, _t(c.mask1, dtype), dtype=dtype, **kw)
    return tr.loss(p, _t(c.feats, dtype), c.tokens, c.norm_B, _t(c.mask1, dtype), _t(c.mask2, dtype), dtype=dtype, **kw)


def sharpen(c, rng, wout_rms):
    """Turn c.model (orc.init_weights) into a trained-like one and c.tokens into targets it mostly predicts; see the module docstring."""
    m = c.model
    for n, k in SHARP_SCALE.items():
        m.p[n] *= np.float32(k)
    for n, r in dict(SHARP_RMS, Wout=wout_rms).items():
        m.p[n] *= np.float32(r / np.sqrt(np.mean(m.p[n].astype(np.float64) ** 2)))
    m.p["bout"][:] = rng.standard_normal(m.p["bout"].shape).astype(np.float32)
    for n in ("b1", "b2"):
        m.p[n] += (0.5 * rng.standard_normal(m.p[n].shape)).astype(np.float32)
    # greedy self-decode of the float64 transcription, teacher-forced on its own (lifted) choices, under the case's masks
    p = torch_params(m)
    step = tr.lrcn1 if c.n_layers == 1 else tr.lrcn
    with torch.no_grad():
        s = [torch.zeros(c.B, m.H1, dtype=torch.float64) for _ in range(2 * c.n_layers)]
        x_cnn = _t(c.feats, torch.float64) @ p["Wcnn"]
        tok = np.full(c.B, tr.BOS)
        for t in range(c.T):
            y = step(p, s, x_cnn, p["Wembed"][torch.as_tensor(tok, dtype=torch.long)], None if c.mask1 is None else _t(c.mask1[t], torch.float64),
                     None if c.mask2 is None else _t(c.mask2[t], torch.float64))
            tok = np.maximum(y.argmax(1).numpy(), 3)
            c.tokens[t] = tok
    # every row's last target is eos, which this model does not predict: those terms count towards the SHARP_MISSES share of misses
    swap = rng.random(c.tokens.shape) < max(0.0, SHARP_MISSES - 1.0 / (c.T + 1)) * (c.T + 1) / c.T
    c.tokens[swap] = rng.integers(3, m.V, size=int(swap.sum()))


def _targets(c):
    """Targets (T + 1, B) and the mask of active loss terms."""
    tgt = np.vstack([c.tokens, np.zeros((1, c.B), np.int32)]).astype(np.int64)
    act = np.ones((c.T + 1, c.B), bool)
    if c.lens is not None:
        steps = np.arange(c.T + 1)[:, None]
        tgt = np.where(steps < c.lens[None, :], tgt, 0)
        act = steps <= c.lens[None, :]
    return tgt, act


def p_target(c, logits):
    """Mean softmax probability of the target over the active loss terms, from float64 logits (T + 1, B, V)."""
    tgt, act = _targets(c)
    pt = np.take_along_axis(torch.softmax(torch.as_tensor(logits), 2).numpy(), tgt[..., None], 2)[..., 0]
    return float(pt[act].mean())


@functools.lru_cache(maxsize=None)
def case(name, regime):
    """The inputs of one case: model (orc.Model), feats, tokens [T][B], mask1 / mask2, lens / norm_tokens, norm_B, pdrop / seed (None unless
    the masks are the device's own, which the GPU test then asks for by (pdrop, seed) and every reference takes as mask1 / mask2)."""
    d = CASES[name]
    c = Case()
    c.name, c.regime = name, regime
    c.E = c.H = d["E"]
    c.V, c.B, c.T, c.n_layers = d["V"], d["B"], d["T"], d.get("n_layers", 2)
    seed = 1000 + 10 * CASE_NUMBER[name] + REGIMES.index(regime)
    for wout_rms in (SHARP_WOUT_RMS if regime == "sharp" else (None,)):   # the mildest rung that reaches the regime: sharp, and no sharper
        c = _build(c, d, seed, wout_rms)
        if wout_rms is None or p_target(c, _forward(c)) >= P_TARGET_MIN:
            break
    c.wout_rms = wout_rms
    return c


def _forward(c):
    logits = []
    with torch.no_grad():
        transcription_loss(c, torch_params(c.model), collect=logits)
    return np.stack([y.numpy() for y in logits])


def _build(c, d, seed, wout_rms):
    rng = np.random.default_rng(seed)
    c.model = orc.init_weights(c.E, c.H, c.H, c.V, seed=seed, n_layers=c.n_layers)
    c.feats = (rng.standard_normal((c.B, 4096)) * 0.05).astype(np.float32)
    c.tokens = rng.integers(3, c.V, size=(c.T, c.B)).astype(np.int32)
    c.mask1 = c.mask2 = c.lens = c.norm_tokens = None
    c.norm_B = d.get("norm_B", c.B)
    c.pdrop, c.seed = d.get("pdrop"), d.get("seed")
    if c.pdrop is not None:   # tests/dropout_ref.py: the host transcription of the device's counter hash
        c.mask1, c.mask2 = dr.masks(c.seed, c.pdrop, c.T, c.B, c.E, c.H, c.n_layers)
    if "keep" in d:
        keep = d["keep"]
        c.mask1 = ((rng.random((c.T + 1, c.B, c.E)) < keep) / keep).astype(np.float32)
        c.mask2 = ((rng.random((c.T + 1, c.B, c.H)) < keep) / keep).astype(np.float32)
    if "lens" in d:
        c.lens = np.asarray(d["lens"], np.int32)
        c.norm_tokens = vr.norm_tokens_of(c.lens)
        assert len(c.lens) == c.B and c.lens.min() == 0 and c.lens.max() == c.T and vr.integer_row_norms(c.lens) is not None
    if wout_rms is not None:
        sharpen(c, rng, wout_rms)
    if c.lens is not None:
        c.tokens = vr.pad_with(c.tokens, c.lens, tr.EOS)   # what the transcription feeds past a row's end; never a loss term
    return c


class Result:
    """loss (float), g (name -> float64 array, absent tensors left out), logits ((T + 1, B, V) float64 or None)."""

    def __init__(self, loss, g, logits=None):
        self.loss, self.g, self.logits = float(loss), g, logits


@functools.lru_cache(maxsize=None)
def reference(name, regime):
    """The float64 transcription of the case: Result with .p_target, .saturated, .max_logit; the sharp regime is asserted here."""
    c = case(name, regime)
    p = torch_params(c.model, requires_grad=True)
    logits, gates = [], []
    val = transcription_loss(c, p, collect=logits, gates=gates)
    val.backward()
    r = Result(val.item(), {n: p[n].grad.numpy().astype(np.float64) for n in p})
    r.logits = np.stack([y.numpy() for y in logits])
    tgt, act = _targets(c)
    r.p_target = p_target(c, r.logits)
    r.saturated = float(np.mean([(g.abs() > 3).double().mean().item() for g in gates]))
    r.max_logit = float(np.abs(r.logits).max())
    # the loss from the float64 logits, max subtracted by hand: ties the logits, the targets and the normaliser to the autograd value
    zs = r.logits - r.logits.max(2, keepdims=True)
    lp = np.take_along_axis(zs, tgt[..., None], 2)[..., 0] - np.log(np.exp(zs).sum(2))
    norm = c.norm_tokens if c.lens is not None else c.norm_B * (c.T + 1)
    assert abs(-(lp * act).sum() / norm - r.loss) <= 1e-12 * abs(r.loss)
    assert np.isfinite(r.logits).all() and np.isfinite(r.loss)
    if regime == "sharp":
        assert r.p_target >= P_TARGET_MIN, (name, "mean p(target)", r.p_target)
        assert r.saturated >= SATURATED_MIN, (name, "share of layer-1 gate pre-activations with |z| > 3", r.saturated)
    return r


@functools.lru_cache(maxsize=None)
def reference_f32(name, regime):
    """The same transcription in torch float32 on the CPU: its distance to reference() is the float32 floor of the case."""
    c = case(name, regime)
    p = torch_params(c.model, torch.float32, requires_grad=True)
    val = transcription_loss(c, p, torch.float32)
    val.backward()
    return Result(val.item(), {n: p[n].grad.numpy().astype(np.float64) for n in p})


@functools.lru_cache(maxsize=None)
def oracle_result(name, regime, emulate=False, fast=False):
    """The C oracle on the case (emulate: under orc.emulate_bf16()); mixed lengths through tests/varlen_ref.py.  Returns (Result, the
    oracle's own gradient object) -- the latter is what parity_util's checks take.  fast: the float-accumulating build with its re-ordered
    GEMMs -- under emulation the same rounding points in another summation order."""
    c = case(name, regime)
    kw = {}
    if fast:
        kw["fast"] = True
        orc.lib(True).orc_set_emulate_bf16(int(emulate))
    try:
        return _oracle(c, emulate, kw)
    finally:
        if fast:
            orc.lib(True).orc_set_emulate_bf16(0)


def _oracle(c, emulate, kw):
    with orc.emulate_bf16(emulate):
        if c.lens is not None:   # row norms norm_tokens / (len + 1): under emulation d(logits) is then rounded at the library's scale
            val, g = vr.loss(c.model, c.feats, c.tokens, c.lens, c.norm_tokens, want_grad=True, row_norms=vr.integer_row_norms(c.lens), **kw)
        else:
            val, g = orc.loss(c.model, c.feats, c.tokens, norm_B=c.norm_B, mask1=c.mask1, mask2=c.mask2, want_grad=True, **kw)
    return Result(val, {n: np.asarray(g.p[n], np.float64) for n in live(c.model)}), g


def rel_norm(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / (np.linalg.norm(ref) + 1e-300))


def distances(res, ref):
    """Per-tensor ||g - g_ref|| / ||g_ref|| and the loss's relative distance."""
    return {n: rel_norm(res.g[n], ref.g[n]) for n in ref.g}, abs(res.loss - ref.loss) / abs(ref.loss)


def digest():
    with open(DIGEST) as f:
        return json.load(f)


def assert_digest(name, regime):
    """The transcription's loss against the committed value: a numpy / torch / init_weights change that alters the inputs fails here."""
    want = digest()["%s/%s" % (name, regime)]
    got = reference(name, regime).loss
    assert abs(got - want) <= 1e-9 * abs(want), (name, regime, got, want)


BEAM_SEED, BEAM_IMAGES, BEAM_NWORD, BEAM_MARGIN = 0, 4, 12, 1.05


@functools.lru_cache(maxsize=None)
def beam_reference(K):
    """beam_search_ref on the sharp C1 model for BEAM_IMAGES images: [(tokens, probability, winner / runner-up)].  The images' seed is
    chosen such that every winner leads by BEAM_MARGIN in float64 (asserted by the CPU test): a float32 product cannot then flip it."""
    c = case("c1", "sharp")
    p = torch_params(c.model)
    out = []
    for f in beam_feats():
        xs = tr.beam_search_ref(p, torch.tensor(f[None], dtype=torch.float64), K, BEAM_NWORD)
        out.append((xs[0][0], float(xs[0][1]), float(xs[0][1]) / float(xs[1][1])))
    return out


def beam_feats():
    return (np.random.default_rng(BEAM_SEED).standard_normal((BEAM_IMAGES, 4096)) * 0.05).astype(np.float32)
