"""The bf16 scoring call of tests/test_gpu_score.py's ride-along tests, shared with its CPU side (tests/test_score_blocks_case.py): edge68 at
V = 300 (tests/width_cases.py: H = 68, every route predicate accepts) on a context of max_B = 256; 300 captions -- 40 of length 6, 8 of
length 1 and 63 each of lengths 2 .. 5 -- 260 images, and 520 pairs in which every caption and every image occurs.

The model is width_cases.decode_model with Wembed x 16 and W1, W2, Wproj, Wout x 4: at decode_model's own scale the word that is FED moves a
score by a hundredth of the bf16 bound (5e-2 + 2e-2 |s|), so a scoring call that feeds caption block 1 the words of block 0 passed that
bound (seen on a deliberately wrong build).  At this scale it moves the median score of block 1 by 3.5 bounds; the CPU test asserts it."""
import functools

import numpy as np

import width_cases as wc
from oracle import oracle as orc

SET, V = "edge68", 300
MAX_B = 256
N_LONG, LONG = 40, 6
SHORT_LENS = np.concatenate([np.full(8, 1), np.repeat([2, 3, 4, 5], 63)])
M, N, P = N_LONG + len(SHORT_LENS), 260, 520


def bound(v):
    """test_bf16_production_matches_emulating_oracle's"""
    return 5e-2 + 2e-2 * abs(v)


@functools.lru_cache(maxsize=None)
def model():
    src = wc.decode_model(SET, V)
    m = orc.Model(src.E, src.H1, src.H2, src.V, {n: a.copy() for n, a in src.p.items()}, src.n_layers)
    m.p["Wembed"] *= 16.0
    for n in ("W1", "W2", "Wproj", "Wout"):
        m.p[n] *= 4.0
    return m


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case():
    c = Case()
    rng = np.random.default_rng(41)
    c.lens = np.concatenate([np.full(N_LONG, LONG), SHORT_LENS])
    rng.shuffle(c.lens)
    wr = np.random.default_rng(42)
    c.caps = [[int(w) for w in wr.integers(3, V, size=int(n))] for n in c.lens]      # no eos / bos / unk inside
    c.feats = (np.random.default_rng(43).standard_normal((N, 4096)) * 0.05).astype(np.float32)
    c.pc = np.concatenate([rng.permutation(M), rng.integers(0, M, size=P - M)])
    c.pi = np.concatenate([rng.permutation(N), rng.permutation(N)])
    c.order = sorted(range(M), key=lambda k: -len(c.caps[k]))                        # score_impl's: by length, descending, stable
    return c


def score(m, feat, inputs, targets, bf16=False):
    """sum_t log softmax(z_t)[y_t] with the step inputs bos, `inputs` and the targets `targets`, eos -- the two are the same words in a
    correct call."""
    Lc = len(targets)
    toks = np.array(inputs, np.int32).reshape(Lc, 1)
    if bf16:
        with orc.emulate_bf16():
            z = orc.forward_logits(m, feat[None], toks)
    else:
        z = orc.forward_logits(m, feat[None], toks)
    z = z.astype(np.float64)[:, 0]
    lse = z.max(axis=1) + np.log(np.exp(z - z.max(axis=1, keepdims=True)).sum(axis=1))
    y = list(targets) + [0]
    return float(sum(z[t, y[t]] - lse[t] for t in range(Lc + 1)))
