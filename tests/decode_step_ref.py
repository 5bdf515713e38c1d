"""One step of the batched decode (decode_begin / decode_step of csrc/decode.hip) for all R rows at once, restated in NumPy float64, with a
DERIVED bound on what a correct f32-accumulating device may differ from it by; the case table of tests/test_gpu_decode_step.py.

The step (lrcn.jl:529-551, :611, :650, :673-676), row r of image r // per_image, input token tok[r], parent row par[r]:
    x      = Wembed[tok]
    a1     = [x | h1[par]] W1 + b1,   gates [f|i|o|g] = [sigm|sigm|sigm|tanh](a1),   c1 = c1[par] f + i g,   h1 = o tanh(c1)
    a2     = [h1 Wproj | x_cnn[image] | h2[par]] W2 + b2,   the same cell -> c2, h2        (x_cnn = feats Wcnn, once per call)
    logits = h2 Wout + bout
LRCN-1f: a1 = [x | x_cnn[image] | h1[par]] W1 + b1 and logits = h1 Wout + bout.

Two modes.  EXACT (the f32 contexts): operands as given.  BF16-EMULATING (the bf16 contexts): every GEMM operand is rounded to bfloat16
exactly where the library rounds it -- the weights, the features, the embedding, x_cnn, the projection h1 Wproj, and h (which the device
already stores as bfloat16) -- sums exact, c, the biases and the tables' sums unrounded.  The three routes of decode_route form the same bf16
products (tables: x W1x + b1 per token and [0 | x_cnn] W2x + b2 per image are summed once per call and added in the cell epilogue), so
one emulation serves all of them.

EACH STEP IS HELD ON ITS OWN, and each layer inside it: the reference's h1[par], c1[par], h2[par], c2[par] are the DEVICE's outputs of the
step before, layer 2 is fed the DEVICE's h1 of this step and the logits its h2 (h1 on LRCN-1f).  Nothing compounds, every operand of every
contraction is known exactly -- except the two the entry does not return, which are bounded instead (4. below).

The bounds (u = 2^-24, the f32 unit roundoff).
1.  A contraction of K real terms plus a bias, summed in f32 in any order:  |a_dev - a| <= gamma(K) (sum_k |x_k w_k| + |b|),
    gamma(K) = (K + 8) 2^-23 -- twice the IEEE worst case K u, because the matrix unit's internal adds are not documented as correctly
    rounded (the fp8 note in tests/test_gpu_vgg_parity.py), and 8 terms for the roundings around the sum (the table entry stored as f32, its
    addition in the epilogue, the bias, the argument of the activation).  K counts both chains on the tables route: E + H1, 2 H2.  The
    zero K padding adds nothing.  sum |x w| is formed exactly per element.
2.  The cell.  sigm has Lipschitz constant 1/4, tanh 1, for any finite perturbation; expf / tanhf / the divide add EPS_ACT = 8 u absolute (4 f32
    ulps of 1, which bounds every activation):
        df = da_f / 4 + EPS_ACT (di, do alike),   dg = da_g + EPS_ACT
        dc = |c_prev| df + |g| di + i dg + di dg + 3 u (|c_prev f| + |i g|)          (two products and a sum in f32)
        dh = |tanh c| do + o (dc + EPS_ACT) + do (dc + EPS_ACT) + u |h|
    with c_prev the device's own value and f, i, o, g, tanh c the reference's.
3.  h in bfloat16.  Rounding is monotone, so the device's h lies in [bf16(h - dh), bf16(h + dh)].  Where the two ends coincide -- the exact h is
    farther than dh from every rounding boundary -- the device's h must BE that value, bit for bit; elsewhere either neighbour is accepted
    (`loose`).  The share of loose entries is a property of the reference alone and is capped at MAX_LOOSE_SHARE = 1/3 for every case.
4.  The operands the device keeps to itself: the projection P = h1 Wproj (K = H1) and x_cnn = feats Wcnn (K = 4096, made once in
    decode_begin).  Either has the error of 1. (dP, dX).  In f32 that error reaches layer 2 as sum_j dx_j |W2[j, col]|.  In bf16 the device
    rounds its own sum, so its operand lies in [bf16(x - dx), bf16(x + dx)]: an entry whose exact value is within dx of a rounding boundary may
    land on either neighbour, `slack_j = max(bf16(x + dx) - bf16(x), bf16(x) - bf16(x - dx))` (one bf16 ulp for the projection, whose dP is far
    below an ulp; 0 for every entry clear of a boundary), and layer 2 gets sum_j slack_j |W2[j, col]| on top of 1; on LRCN-1f x_cnn's term
    enters layer 1.
    THE FEATURES ARE SPARSE BECAUSE OF THIS.  With dense 0.05 N(0,1) features the 4096-term bound is dX = gamma(4096) sum |f w| ~ 5e-4 * 3
    ~ 9e-4 (the f32 sum's real error is ~2e-8), which is four bf16 ulps of x_cnn ~ 0.03: EVERY entry of x_cnn would carry slack, layer 2's
    bound would grow a hundredfold to ~1e-3 and 100 % of h2 would be loose (measured on tables-260; without x_cnn's slack 3.5 %).  The cap
    of 3. is a condition, so the inputs change, not the cap: every image's features are 0.05 N(0,1) on FEAT_NNZ = 32 coordinates -- the
    first and the last of the 4096 always among them, so that both ends of the K loop carry weight -- and zero elsewhere.  A zero feature
    contributes an exact zero to any partial sum in any order, so the contraction has K = 32 real terms, dX ~ 1e-7 against an ulp of
    ~1e-5, and about one entry in thirty carries slack.  x_cnn ~ 3e-3 still moves a layer-2 pre-activation by ~1e-3 when a row reads
    another image's, a hundred times that layer's bound.
5.  logits: 1. with K = H2 (H1 on LRCN-1f) on the device's own h.
"""
import numpy as np

from oracle import oracle as orc

V = 301
STEPS = 3
U = 2.0 ** -24
EPS_ACT = 8 * U
MAX_LOOSE_SHARE = 1.0 / 3.0
FEAT_NNZ = 32
ROUTE_NAMES = ("plain", "epi", "tables")

# id -> (bf16, layers, E, H1, H2, N, per_image, knob or None, route); tests/INSTANTIATIONS.md "Batched decode step" names these ids
CASES = {
    "tables-260":   (True, 2, 40, 72, 136, 52, 5, None, "tables"),    # 4-row tail in the 2nd row block; 4H = 288 / 544: column tiles 128+128+32; H1 != H2
    "tables-515":   (True, 2, 40, 72, 136, 103, 5, None, "tables"),   # three row blocks
    "tables-68":    (True, 2, 40, 68, 68, 86, 3, None, "tables"),     # H % 8 == 4: scalar tails of k_decode_prep_h; h = 34
    "epi-by-width": (True, 2, 40, 64, 64, 52, 5, None, "epi"),        # H = 64: the tables rule's own boundary (> 64)
    "epi-knob":     (True, 2, 40, 72, 136, 52, 5, "LRCN_DECODE_TABLES", "epi"),   # same inputs as tables-260
    "epi-1f":       (True, 1, 37, 72, 72, 64, 4, None, "epi"),        # exactly 256 rows; E % 8 != 0: the embedding copy stops at E, x_cnn right behind it
    "plain-255":    (True, 2, 40, 72, 136, 51, 5, None, "plain"),     # one row below the 256 rule
    "plain-h70":    (True, 2, 40, 70, 136, 52, 5, None, "plain"),     # H1 % 4 != 0
    "plain-knob":   (True, 2, 40, 72, 136, 52, 5, "LRCN_DECODE_EPI", "plain"),    # same inputs as tables-260
    "plain-f32":    (False, 2, 40, 72, 136, 52, 5, None, "plain"),    # exact-fp32 path, exact reference
    "plain-f32-1f": (False, 1, 37, 72, 72, 20, 3, None, "plain"),     # LRCN-1f, small
    # two rungs the audit for tests/INSTANTIATIONS.md found beside the eleven above
    "epi-68-knob":  (True, 2, 40, 68, 68, 86, 3, "LRCN_DECODE_TABLES", "epi"),    # tables-68's inputs: k_decode_prep's scalar tails of h1 / h2 (H % 8 == 4)
    "plain-1f-knob": (True, 1, 37, 72, 72, 64, 4, "LRCN_DECODE_EPI", "plain"),    # epi-1f's inputs: the plain step in bf16 on LRCN-1f
}
SAME_INPUT = ("tables-260", "epi-knob", "plain-knob")
KNOBS = ("LRCN_DECODE_TABLES", "LRCN_DECODE_EPI")


def predict_route(case):
    """decode_route's rule (csrc/decode.hip decode_epi_on / decode_tables_on), restated."""
    bf16, layers, _, H1, H2, N, per_image, knob, _ = CASES[case]
    epi = knob != "LRCN_DECODE_EPI" and bf16 and N * per_image >= 256 and H1 % 4 == 0 and H2 % 4 == 0
    tables = epi and knob != "LRCN_DECODE_TABLES" and layers == 2 and H1 > 64 and H2 > 64
    return "tables" if tables else "epi" if epi else "plain"


def gamma(K):
    return (K + 8) * 2.0 ** -23


def bf16_round64(x):
    """float64 -> the nearest bfloat16 (ties to even), as float64: one rounding, not through float32."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    q = np.ldexp(1.0, e - 8)          # the spacing of 8-bit significands in x's binade
    return np.rint(x / q) * q         # np.rint rounds half to even; x / q and the product are exact


def sigm(a):
    return 1.0 / (1.0 + np.exp(-a))


# ------------------------------------------------------------------------------------------------------------------------ inputs
def make_inputs(case):
    """(model, feats [N][4096] f32, tokens [STEPS][R] i32, parents [STEPS][R] i32) of a case: a function of its shape alone, so the
    SAME_INPUT cases get identical inputs."""
    bf16, layers, E, H1, H2, N, per_image, _, _ = CASES[case]
    R = N * per_image
    rng = np.random.default_rng([layers, E, H1, H2, N, per_image])
    m = orc.init_weights(E, H1, H2, V, seed=11, n_layers=layers)
    if layers == 2:
        m.p["b2"][:] = (rng.standard_normal(m.p["b2"].shape) * 0.5).astype(np.float32)    # a lost bias cannot hide
    m.p["bout"][:] = (rng.standard_normal(m.p["bout"].shape) * 0.5).astype(np.float32)
    feats = np.zeros((N, orc.CNNOUT), np.float32)                 # 0.05 N(0,1) on FEAT_NNZ coordinates per image (4. of the module docstring)
    for n in range(N):
        at = np.concatenate([[0, orc.CNNOUT - 1], 1 + rng.choice(orc.CNNOUT - 2, FEAT_NNZ - 2, replace=False)])   # both ends of K, always
        feats[n, at] = (rng.standard_normal(FEAT_NNZ) * 0.05).astype(np.float32)
    tokens = rng.integers(0, V, size=(STEPS, R)).astype(np.int32)
    tokens[:, 0], tokens[:, 1] = 0, V - 1
    tokens[:, 3] = tokens[:, 2]                                   # a repeated token
    parents = rng.integers(0, R, size=(STEPS, R)).astype(np.int32)    # arbitrary rows, not confined to the row's image
    parents[0] = -1                                               # never read (and refused if it were: the entry checks steps >= 1 only)
    for s in range(1, STEPS):
        parents[s, 0], parents[s, 7] = 0, 7                       # fixed points
        parents[s, 5] = parents[s, 6] = 9 + s                     # a repeated parent
        parents[s, 3], parents[s, R - 1] = R - 2, 2               # first rows <-> last rows
        if R > 256:                                               # across the 256-row block boundary, both directions
            parents[s, 255], parents[s, 256] = 256, 255
            parents[s, 10 + s], parents[s, 257] = 257, 11
    return m, feats, tokens, parents


def crosses_blocks(parents, R):
    up = any(r < 256 <= p for s in range(1, STEPS) for r, p in enumerate(parents[s]))
    down = any(p < 256 <= r for s in range(1, STEPS) for r, p in enumerate(parents[s]))
    return up and down


# ------------------------------------------------------------------------------------------------------------------------ the reference
class Ref:
    """The per-call part: operands in float64 (bf16: rounded where the library rounds them), x_cnn with its error bound and slack."""

    def __init__(self, model, feats, per_image, bf16):
        self.bf16, self.two = bool(bf16), model.n_layers == 2
        self.E, self.H1, self.H2, self.h = model.E, model.H1, model.H2, model.H2 // 2
        rw = bf16_round64 if bf16 else (lambda a: np.asarray(a, np.float64))
        p = {n: np.asarray(model.p[n], np.float64) for n in orc.PARAM_NAMES}
        self.W1, self.W2, self.Wproj, self.Wemb, self.Wout = rw(p["W1"]), rw(p["W2"]), rw(p["Wproj"]), rw(p["Wembed"]), rw(p["Wout"])
        self.b1, self.b2, self.bout = p["b1"].reshape(-1), p["b2"].reshape(-1), p["bout"].reshape(-1)
        F, Wc = rw(feats), rw(p["Wcnn"])
        self.per_image = per_image
        x = F @ Wc                                                           # [N][h]  (lrcn.jl:611)
        dx = gamma(np.count_nonzero(F, axis=1))[:, None] * (np.abs(F) @ np.abs(Wc))   # a zero feature adds an exact zero: K = the non-zero terms
        self.xcnn, self.xcnn_slack = self.operand(x, dx)

    def operand(self, x, dx):
        """What the device feeds its next contraction for an intermediate it computed itself as x +- dx, and how far that may lie from
        the value returned here (4. of the module docstring)."""
        if not self.bf16:
            return x, dx
        r = bf16_round64(x)
        return r, np.maximum(bf16_round64(x + dx) - r, r - bf16_round64(x - dx))

    def gates(self, xh, W, b, slack, n_slack_rows_from):
        """a = xh W + b and its bound; `slack` [R][n] bounds the device's deviation in the operand columns from n_slack_rows_from on."""
        a = xh @ W + b
        S = np.abs(xh) @ np.abs(W) + np.abs(b)
        da = gamma(W.shape[0]) * S
        if slack is not None:
            j0 = n_slack_rows_from
            prop = slack @ np.abs(W[j0:j0 + slack.shape[1]])
            da = da + (1.0 + gamma(W.shape[0])) * prop
        return a, da

    @staticmethod
    def cell(a, da, c_prev):
        H = a.shape[1] // 4
        f, i, o, g = sigm(a[:, :H]), sigm(a[:, H:2 * H]), sigm(a[:, 2 * H:3 * H]), np.tanh(a[:, 3 * H:])
        df, di, do = (da[:, k * H:(k + 1) * H] / 4 + EPS_ACT for k in range(3))
        dg = da[:, 3 * H:] + EPS_ACT
        c = c_prev * f + i * g
        dc = np.abs(c_prev) * df + np.abs(g) * di + i * dg + di * dg + 3 * U * (np.abs(c_prev * f) + np.abs(i * g))
        tc = np.tanh(c)
        dtc = dc + EPS_ACT
        h = o * tc
        dh = np.abs(tc) * do + o * dtc + do * dtc + U * np.abs(h)
        return c, dc, h, dh

    def h_window(self, h, dh):
        """[lo, hi] the device's stored h must lie in; bf16: the roundings of h -+ dh (lo == hi: bit-exact)."""
        if self.bf16:
            return bf16_round64(h - dh), bf16_round64(h + dh)
        return h - dh, h + dh

    def step(self, tok, prev, h1_dev=None, h2_dev=None):
        """One step for all rows.  prev: None (first step: zero states) or the dict {"h1","c1","h2","c2"} [R][H] ALREADY gathered by the
        parents.  h1_dev / h2_dev: the device's h of THIS step ([R][H]; None: the reference's own h as the device would store it -- the CPU
        simulation).  Returns c1, dc1, h1_lo, h1_hi, c2, dc2, h2_lo, h2_hi, logits, dlogits (layer 2's None on LRCN-1f) and h1, h2."""
        R = len(tok)
        img = np.arange(R) // self.per_image
        z = lambda H: np.zeros((R, H))  # noqa: E731
        prev = prev or {"h1": z(self.H1), "c1": z(self.H1), "h2": z(self.H2), "c2": z(self.H2)}
        emb = self.Wemb[tok]
        out = {}
        if self.two:
            a1, da1 = self.gates(np.hstack([emb, prev["h1"]]), self.W1, self.b1, None, 0)
        else:
            a1, da1 = self.gates(np.hstack([emb, self.xcnn[img], prev["h1"]]), self.W1, self.b1, self.xcnn_slack[img], self.E)
        out["c1"], out["dc1"], h1, dh1 = self.cell(a1, da1, prev["c1"])
        out["h1_lo"], out["h1_hi"] = self.h_window(h1, dh1)
        store = bf16_round64 if self.bf16 else (lambda a: a)
        h1_dev = store(h1) if h1_dev is None else np.asarray(h1_dev, np.float64)
        out["h1"], h_last, H_last = h1_dev, h1_dev, self.H1
        if self.two:
            P = h1_dev @ self.Wproj                                           # lrcn.jl:544
            Pr, P_slack = self.operand(P, gamma(self.H1) * (np.abs(h1_dev) @ np.abs(self.Wproj)))
            x2, slack = np.hstack([Pr, self.xcnn[img]]), np.hstack([P_slack, self.xcnn_slack[img]])
            a2, da2 = self.gates(np.hstack([x2, prev["h2"]]), self.W2, self.b2, slack, 0)
            out["c2"], out["dc2"], h2, dh2 = self.cell(a2, da2, prev["c2"])
            out["h2_lo"], out["h2_hi"] = self.h_window(h2, dh2)
            h2_dev = store(h2) if h2_dev is None else np.asarray(h2_dev, np.float64)
            out["h2"], h_last, H_last = h2_dev, h2_dev, self.H2
        out["logits"] = h_last @ self.Wout + self.bout                       # lrcn.jl:550
        out["dlogits"] = gamma(H_last) * (np.abs(h_last) @ np.abs(self.Wout) + np.abs(self.bout))
        return out

    def loose_share(self, out):
        """Share of this step's h entries that get the either-neighbour allowance (bf16) -- from the reference alone."""
        n = loose = 0
        for k in ("h1", "h2") if self.two else ("h1",):
            loose += int(np.count_nonzero(out[k + "_lo"] != out[k + "_hi"]))
            n += out[k + "_lo"].size
        return loose / n


def gather(dev, s, parents):
    """The device's states after step s - 1, gathered by parents[s]: step s's inputs (None for the first step)."""
    if s == 0:
        return None
    return {k: None if dev[k] is None or dev[k][s - 1] is None else np.asarray(dev[k][s - 1], np.float64)[parents[s]]
            for k in ("h1", "c1", "h2", "c2")}


def check_step(ref, out, dev, s):
    """Assert the device's step-s outputs against `out` = ref.step(...) fed the device's inputs; returns the figures it asserted on
    (worst ratio error / bound per quantity, the loose share)."""
    fig = {}

    def bounded(k, dk):
        err = np.abs(np.asarray(dev[k][s], np.float64) - out[k])
        fig[k] = float((err / out[dk]).max())
        bad = np.argwhere(err > out[dk])
        assert bad.size == 0, "step %d %s: %d of %d entries outside the bound, first at %s: device %r, reference %r, bound %.3g" % (
            s, k, len(bad), err.size, tuple(bad[0]), float(dev[k][s][tuple(bad[0])]), float(out[k][tuple(bad[0])]), float(out[dk][tuple(bad[0])]))

    def windowed(k):
        hd = np.asarray(dev[k][s], np.float64)
        lo, hi = out[k + "_lo"], out[k + "_hi"]
        bad = np.argwhere((hd < lo) | (hd > hi))
        fig[k + "_firm"] = float(np.mean(lo == hi))
        assert bad.size == 0, "step %d %s: %d of %d entries outside [lo, hi] (%d of them where lo == hi: bit-exact), first at %s: device %r, window [%r, %r]" % (
            s, k, len(bad), hd.size, int(np.count_nonzero((lo == hi)[tuple(bad.T)])), tuple(bad[0]), float(hd[tuple(bad[0])]), float(lo[tuple(bad[0])]),
            float(hi[tuple(bad[0])]))

    bounded("c1", "dc1")
    windowed("h1")
    if ref.two:
        bounded("c2", "dc2")
        windowed("h2")
    bounded("logits", "dlogits")
    fig["loose"] = ref.loose_share(out)
    if ref.bf16:
        assert fig["loose"] < MAX_LOOSE_SHARE, "step %d: %.1f %% of h gets the either-neighbour allowance" % (s, 100 * fig["loose"])
    return fig


def check_case(ref, dev, tokens, parents):
    """Every step of a device run, each held on its own; returns the per-step figures."""
    figs = []
    for s in range(len(tokens)):
        out = ref.step(tokens[s], gather(dev, s, parents), dev["h1"][s], dev["h2"][s] if ref.two else None)
        figs.append(check_step(ref, out, dev, s))
    return figs


def simulate(ref, tokens, parents):
    """A stand-in device on the CPU: the reference run forward on its own outputs (h as the device stores it, c and logits in f32)."""
    keys = ("h1", "c1", "h2", "c2", "logits")
    dev = {k: [] for k in keys}
    for s in range(len(tokens)):
        out = ref.step(tokens[s], gather(dev, s, parents))
        for k in keys:
            v = out.get(k)
            dev[k].append(None if v is None else v.astype(np.float32).astype(np.float64))
    return {k: (None if v[0] is None else np.stack(v)) for k, v in dev.items()}
