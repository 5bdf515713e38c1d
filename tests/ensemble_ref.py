"""Host restatement of the ensemble mixture of include/lrcn_ensemble.h.

`mix(zs, w, mode)` is the definition in float64; `mix_f32` restates the kernel's arithmetic of csrc/ensemble.hip in float32.
`EnsembleStep(steps, w, mode)` wraps member step callables of the nbest_ref kind (step(requests) -> (logits, handles)) into one such
callable whose logits are the mixture rows: every member keeps its own handles and a row's handle is the tuple of them, so
nbest_ref.search, constrained_ref.search and constrained_ref.search_diverse run on an ensemble unchanged.
"""
import numpy as np

PROB, LOGPROB = "prob", "logprob"


def weights(w, M):
    """the weights as the library holds them: None is uniform; normalised in double to sum 1, then rounded to float32"""
    w = np.ones(M, np.float64) if w is None else np.asarray(w, np.float64)
    assert w.shape == (M,) and np.all(np.isfinite(w)) and np.all(w > 0)
    return (w / w.sum()).astype(np.float32)


def log_softmax64(z):
    z = np.asarray(z, np.float64)
    d = z - z.max(axis=-1, keepdims=True)
    return d - np.log(np.exp(d).sum(axis=-1, keepdims=True))


def mix(zs, w, mode):
    """zs: M arrays [R][V] (or [V]) of logits -> the mixture rows, float64.  w as the library holds them (weights())."""
    w = np.asarray(w, np.float32).astype(np.float64)
    lp = np.stack([log_softmax64(z) for z in zs])                     # [M][...][V]
    wb = w.reshape((-1,) + (1,) * (lp.ndim - 1))
    if mode == LOGPROB:
        return (wb * lp).sum(axis=0)
    assert mode == PROB
    mx = lp.max(axis=0)
    return mx + np.log((wb * np.exp(lp - mx)).sum(axis=0))


def mix_f32(zs, w, mode):
    """The kernel's formula with every intermediate rounded to float32, summed in member order (its exp and log are float32 results of
    exact functions here; the kernel's hardware approximations and its per-thread summation order are not restated)."""
    f = np.float32
    w = np.asarray(w, f)
    lps = []
    for z in zs:
        z = np.asarray(z, f)
        d = (z - z.max(axis=-1, keepdims=True)).astype(f)
        se = np.exp(d).astype(f).sum(axis=-1, keepdims=True, dtype=f)
        lps.append((d - np.log(se).astype(f)).astype(f))
    if mode == LOGPROB:
        s = np.zeros_like(lps[0])
        for wm, lp in zip(w, lps):
            s = (s + (wm * lp).astype(f)).astype(f)
        return s
    assert mode == PROB
    mx = lps[0]
    for lp in lps[1:]:
        mx = np.maximum(mx, lp)
    s = np.zeros_like(mx)
    for wm, lp in zip(w, lps):
        s = (s + (wm * np.exp((lp - mx).astype(f)).astype(f)).astype(f)).astype(f)
    return (mx + np.log(s).astype(f)).astype(f)


MIX_R = 7
MIX_V = [20, 203, 1027, 4100, 10640, 16388, 20004]   # below one column group per thread .. two passes of 256 threads x 4 and tails of 1..3
MIX_M = [1, 2, 3, 8]
MIX_SCALES = [1.0, 8.0, 40.0]
MIX_TOL = 1e-5   # |x - ref| <= MIX_TOL (1 + |ref|): the project's tolerance for this arithmetic (check_rows, test_gpu_nbest.compare)


def mix_inputs(V, M, scale):
    """The mix tests' members: seeded normal logits times `scale`, column 3 at -1e4 in member 0 alone and column V - 2 at -1e4 in every
    member; unequal weights 1 .. M (not normalised)."""
    rng = np.random.default_rng([V, M, int(scale)])
    zs = [(rng.standard_normal((MIX_R, V)) * scale).astype(np.float32) for _ in range(M)]
    zs[0][:, 3] = -1e4
    for z in zs:
        z[:, V - 2] = -1e4
    return zs, [float(m + 1) for m in range(M)]


def mix_error(x, ref):
    """the worst |x - ref| / (1 + |ref|)"""
    ref = np.asarray(ref, np.float64)
    return float(np.max(np.abs(np.asarray(x, np.float64) - ref) / (1.0 + np.abs(ref))))


class EnsembleStep:
    """step(requests) over M member steps: requests[q] = (image, handle or None, token), the handle a tuple of the members' handles."""

    def __init__(self, steps, w, mode, mixer=mix):
        self.steps, self.mode, self.mixer = list(steps), mode, mixer
        self.w = weights(w, len(self.steps))

    def __call__(self, req):
        zs, hs = [], []
        for m, step in enumerate(self.steps):
            z, h = step([(n, None if hd is None else hd[m], tok) for n, hd, tok in req])
            zs.append(np.asarray(z, np.float32))
            hs.append(h)
        x = np.asarray(self.mixer(zs, self.w, self.mode)).astype(np.float32)
        return x, [tuple(h[q] for h in hs) for q in range(len(req))]


E2E_N, E2E_NWORD, E2E_W = 8, 12, (0.7, 0.3)   # the end-to-end tests' images, caption length and weights


def e2e_members(orc):
    """The end-to-end tests' two members: test_gpu_nbest.small_model(n_layers=2, seed=3) and a one-layer model of another seed, V = 203."""
    out = []
    for n_layers, seed in ((2, 3), (1, 5)):
        m = orc.init_weights(64, 64, 64, 203, seed=seed, n_layers=n_layers)
        m.p["Wout"][:] *= 16.0
        out.append(m)
    return out


def e2e_feats():
    return (np.random.default_rng(7).standard_normal((E2E_N, 4096)) * 0.05).astype(np.float32)   # test_gpu_nbest.feats_of(8, 7)
