"""Host restatement of scheduled sampling (include/lrcn_sched.h), tests only: the coin in numpy float32, the draw through philox_ref, the
caption model with SEPARATE inputs and targets on tests/torch_ref.py's lrcn / lrcn1 steps in float64 autograd (lens, row weights, masks),
and a full sequential simulation.  Nothing here comes from the HIP sources.

The GPU tests never compare with the simulation end to end (two chains may part ways at a near tie): they check every coin exactly, every
draw against the DEVICE's logits row of the step before, and loss / gradients / logits under the DEVICE's fed words.  The simulation serves
the host tests: it shows that the seeded cases hold enough draws and few enough near ties for the caps the GPU test applies."""
import numpy as np
import torch

import nucleus_ref as nr
import philox_ref as ph
import torch_ref as tr
from oracle import oracle as orc

EOS, BOS = 0, 1
F64 = torch.float64
MIN_DRAWS = 200        # checked draws per case, pooled over the case's calls
EXCUSED_SHARE = 0.02   # at most this share of them may be near ties (nucleus_ref.excused)

# The seeded cases of tests/test_gpu_sched.py's coin / draw check: name -> (dtype, n_layers, B, T, E, H, V, eps, temperature, row0, mixed lens,
# calls).  `calls` seeds are pooled so that a case holds at least MIN_DRAWS draws (tests/test_sched_host.py counts them in the simulation).
CASES = {
    "f32-eps.5-t1": ("f32", 2, 13, 7, 52, 36, 97, 0.5, 1.0, 0, True, 14),
    "f32-eps1-t0-row1000": ("f32", 2, 13, 7, 52, 36, 97, 1.0, 0.0, 1000, False, 3),
    "f32-1layer-eps1-t1-row1000": ("f32", 1, 11, 6, 40, 48, 203, 1.0, 1.0, 1000, False, 4),
    "bf16-B48-eps.5-t1": ("bf16", 2, 48, 5, 64, 64, 157, 0.5, 1.0, 0, False, 3),
    "f32-V16400-eps1-t1": ("f32", 2, 6, 3, 16, 16, 16400, 1.0, 1.0, 1000, False, 13),
    # k_sched_next_input keeps a logits row of up to 15360 columns in LDS: the last staged width, the first unstaged one, and the unstaged
    # form in bf16
    "f32-V15360-eps1-t1": ("f32", 2, 6, 3, 16, 16, 15360, 1.0, 1.0, 1000, False, 13),
    "f32-V15361-eps1-t1": ("f32", 2, 6, 3, 16, 16, 15361, 1.0, 1.0, 1000, False, 13),
    "bf16-V16400-eps1-t1": ("bf16", 2, 6, 3, 16, 16, 16400, 1.0, 1.0, 1000, False, 13),
}
# The generator seed of a case's inputs, minus 100.  (The first five are the cases' ranks in the sorted table of when there were five: a new
# case takes the next number and moves nobody's inputs.)
_INPUT_SEED = {"bf16-B48-eps.5-t1": 0, "f32-1layer-eps1-t1-row1000": 1, "f32-V16400-eps1-t1": 2, "f32-eps.5-t1": 3, "f32-eps1-t0-row1000": 4,
               "f32-V15360-eps1-t1": 5, "f32-V15361-eps1-t1": 6, "bf16-V16400-eps1-t1": 7}
# Cases whose model carries an output bias on the LAST word, bout[V - 1] = log((V - 1) / 3): with the small logits of init_weights the word
# holds about a quarter of every row's mass, so a kernel that loses the last column of a row (a staged copy that stops one short, a strided
# loop with the wrong bound) draws other words than the host.  tests/test_sched_host.py asserts the share and that the host draws the word.
LAST_COLUMN_CASES = ("f32-V15360-eps1-t1", "f32-V15361-eps1-t1", "bf16-V16400-eps1-t1")
LAST_COLUMN_SHARE = (0.1, 0.5)


def case_inputs(name):
    """(model, feats, tokens, lens, [seeds]) of a case -- the same arrays on the host and in the GPU test."""
    dtype, nl, B, T, E, H, V, eps, temp, row0, mixed, calls = CASES[name]
    rng = np.random.default_rng(_INPUT_SEED[name] + 100)
    m = orc.init_weights(E, H, H, V, seed=B + T, n_layers=nl)
    if name in LAST_COLUMN_CASES:
        m.p["bout"][0, V - 1] = np.float32(np.log((V - 1) / 3.0))
    feats = (rng.standard_normal((B, 4096)) * 0.02).astype(np.float32)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    lens = np.full(B, T, np.int32)
    if mixed:
        lens = rng.integers(0, T + 1, size=B).astype(np.int32)
        lens[0], lens[1] = T, 0
    return m, feats, tokens, lens, [1000003 * (k + 1) + (k << 40) for k in range(calls)]


# ------------------------------------------------------------------------------------------------ coin and draw
def coin_u(seed, s, rows):
    """u of step s for the global rows `rows`: word 0 of Philox counter (0xFFFFFFFF, s, 0xFFFFFFFF, row), float32."""
    rows = np.asarray(rows, dtype=np.int64)
    x = ph.philox4x32_10(np.uint32(0xFFFFFFFF), np.uint32(s), np.uint32(0xFFFFFFFF), (rows & 0xFFFFFFFF).astype(np.uint32),
                         np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))[0]
    return ((x >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def coins(seed, eps, lens, T, row0):
    """fire[s][b] (bool, (T+1, B)): the coin of an eligible (1 <= s <= lens[b]) input fired."""
    lens = np.asarray(lens)
    B = lens.shape[0]
    fire = np.zeros((T + 1, B), bool)
    for s in range(1, T + 1):
        fire[s] = (coin_u(seed, s, row0 + np.arange(B)) < np.float32(eps)) & (s <= lens)
    return fire


def draw_scores(z, temperature, seed, row, s):
    """(columns, float32 scores) of the draw of input (s, row) from the logits row z of step s - 1."""
    return ph.scores(np.asarray(z, np.float32), temperature, 0, seed, i=row & 0xFFFFFFFF, s=0, current=s)


def draw(z, temperature, seed, row, s):
    return ph.draw(np.asarray(z, np.float32), temperature, 0, seed, i=row & 0xFFFFFFFF, s=0, current=s)


def gold_inputs(tokens, lens):
    """tok_in of the padded batch: bos, the gold words, eos past a row's end."""
    tokens = np.asarray(tokens)
    T, B = tokens.shape
    fed = np.zeros((T + 1, B), np.int32)
    fed[0] = BOS
    for s in range(1, T + 1):
        fed[s] = np.where(s <= np.asarray(lens), tokens[s - 1], EOS)
    return fed


# ------------------------------------------------------------------------------------------------ the model under given inputs
class Grads:
    def __init__(self, p):
        self.p = p


def _params(model, want_grad):
    return {n: torch.tensor(np.asarray(model.p[n]), dtype=F64, requires_grad=want_grad) for n in orc.PARAM_NAMES if np.asarray(model.p[n]).size}


def _stepper(p):
    two = "W2" in p
    H1 = p["Wproj"].shape[0] if two else p["Wout"].shape[0]
    H2 = p["Wout"].shape[0]
    return (tr.lrcn, (H1, H1, H2, H2)) if two else (tr.lrcn1, (H1, H1))


def _m(mask, t):
    return None if mask is None else torch.as_tensor(np.asarray(mask[t]), dtype=F64)


def loss(model, feats, tokens, lens, fed, norm_tokens=None, row_w=None, mask1=None, mask2=None, want_grad=False, collect=None):
    """-(1 / norm_tokens) sum_b w_b sum_{s <= lens[b]} log p_{s,b}[gold target], the step inputs being fed[s] ((T+1, B) ids) and NOT the
    gold words.  collect: a list that receives the (B, V) float64 logits of every step.  -> loss, or (loss, Grads)."""
    tokens, lens, fed = np.asarray(tokens), np.asarray(lens), np.asarray(fed)
    T, B = tokens.shape
    p = _params(model, want_grad)
    step, state = _stepper(p)
    s = [torch.zeros(B, H, dtype=F64) for H in state]
    x_cnn = torch.as_tensor(np.asarray(feats), dtype=F64) @ p["Wcnn"]
    w = torch.ones(B, dtype=F64) if row_w is None else torch.as_tensor(np.asarray(row_w, np.float32), dtype=F64)
    ln = torch.as_tensor(lens, dtype=torch.long)
    total = 0.0
    for t in range(T + 1):
        y = step(p, s, x_cnn, p["Wembed"][torch.as_tensor(fed[t], dtype=torch.long)], _m(mask1, t), _m(mask2, t))
        if collect is not None:
            collect.append(y.detach().numpy())
        tgt = torch.as_tensor(tokens[t] if t < T else np.zeros(B), dtype=torch.long)
        tgt = torch.where(t < ln, tgt, torch.full_like(tgt, EOS))
        total = total + (torch.log_softmax(y, 1)[torch.arange(B), tgt] * (t <= ln).to(F64) * w).sum()
    nt = int(lens.astype(np.int64).sum()) + B if norm_tokens is None else int(norm_tokens)
    val = -total / nt
    if not want_grad:
        return float(val)
    val.backward()
    g = {n: (p[n].grad.numpy() if n in p and p[n].grad is not None else np.zeros(np.asarray(model.p[n]).shape)) for n in orc.PARAM_NAMES}
    return float(val.detach()), Grads(g)


def simulate(model, feats, tokens, lens, eps, temperature, seed, row0, mask1=None, mask2=None):
    """The whole chain on the host: step s's logits (float64, cast to float32 for the draw) decide input s + 1.
    -> fed (T+1, B), logits (T+1, B, V) float32, fire (T+1, B), number of near-tie draws (nucleus_ref.excused; temperature 0: exact ties
    are decided by the lowest column on both sides, so none is counted)."""
    tokens, lens = np.asarray(tokens), np.asarray(lens)
    T, B = tokens.shape
    p = _params(model, False)
    step, state = _stepper(p)
    fed = gold_inputs(tokens, lens)
    fire = coins(seed, eps, lens, T, row0)
    s = [torch.zeros(B, H, dtype=F64) for H in state]
    x_cnn = torch.as_tensor(np.asarray(feats), dtype=F64) @ p["Wcnn"]
    logits, near = [], 0
    with torch.no_grad():
        for t in range(T + 1):
            y = step(p, s, x_cnn, p["Wembed"][torch.as_tensor(fed[t], dtype=torch.long)], _m(mask1, t), _m(mask2, t))
            z = y.numpy().astype(np.float32)
            logits.append(z)
            if t < T:
                for b in np.nonzero(fire[t + 1])[0]:
                    cols, sc = draw_scores(z[b], temperature, seed, row0 + int(b), t + 1)
                    fed[t + 1, b] = int(cols[np.argmax(sc)])
                    near += bool(temperature > 0 and nr.excused(sc))
    return fed, np.stack(logits), fire, near
