"""GPU: the embedding-gradient chain of csrc/train_kernels.hip (rank_token_rows, embed_segsum, embed_scatter_rm, embed_stage_to_grad,
embed_rows_export) against exact host references (tests/embed_grad_ref.py, tests/dropout_ref.py).

B1  The ordered form through L.embed_grad_from_rows, every case of the table.  The gradient lives inside a larger device buffer of NaN with a
    lead-in and a guard behind V*E that must stay NaN; no memset precedes the call, so every element of the gradient must be written.
    `int` cases: np.array_equal with the float64 reference (integers below 2^24: exact in any order), the zeros of untouched tokens
    included.  `real` cases: per element |got - ref| <= n_seg 2^-24 sum|x_i| (embed_grad_ref.bound: derived).  Contexts are shared between
    the cases of one (E, V), so every case but the first also starts from the staging array the previous call left behind.
B2  The staging array is zero again on exit: token set A, the disjoint set B (exact, zeros at A's tokens), A again.
B3  Both routes inside lossgradient at the benchmark's width (f32, E = H = 1000, V = 10640, B = 256, T = 11, Zipf targets, pdrop 0.4 by seed):
    the rows lossgradient exports (set_embed_rows_buffer) are bit-identical between two calls, asserted; the reference is their float64 sum
    per exported id; grads[6] without the buffer is held to the B1 bound with n_seg + 1 (the mask multiply may or may not be fused into the
    add), by float atomics (DETERMINISTIC = 0, embed_scatter_rm_kernel) and by rank + segsum (DETERMINISTIC = 1).
B4  The exported rows carry the mask: exactly 0 wherever the host transcription of the counter hash drops, and non-zero in all but 0.1 % of
    the elements it keeps -- which, with the kept share asserted in tests/test_dropout_ref.py, is the on-device unbiasedness check.

Measured on an MI355X, next to the derived bounds (each test prints its own figures).  B1 `real`: the 8192-row segment max |d| 1.2e-4, under
1e-4 of its bound; the 513-row segment case max |d| 1.3e-5, the closest element at 0.54 of its bound; Zipf at E = 1000 / V = 10640 max |d|
1.0e-5, closest 0.59 (the close ones are tokens with two or three rows, where the bound is two or three roundings).  B3: max |ref| 1.3e-5,
max |d| 5.2e-12 by atomics and 1.4e-12 ordered, the closest element at 0.46 of its bound in both; the busiest word owns 305 rows.  B4: 0.5997
of the exported elements are non-zero, exactly the host mask's kept share, and no kept element is zero.  E = 70 is accepted by Context.
Deliberately wrong builds (never committed): embed_segsum skipping the last partial 512-chunk fails B1 at the 513- and 1025-row segments
and the 8192-row Zipf case; `j <= m` in the rank kernel fails every B1 case it was run on (rows below 8192 only: at 8192 it would write one
key past the buffer); embed_stage_to_grad not restoring the zeros fails B2 and six B1 cases that share a context; (b, s) swapped in
embed_segsum's drop_mult fails B3 `ordered`.
"""
import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

import dropout_ref as dr
import embed_grad_ref as er

pytestmark = pytest.mark.gpu
F32 = lrcn_amd.LRCN_F32
LEAD, GUARD = 64, 4096   # floats of NaN before (a multiple of 4: the gradient stays 16-byte aligned) and behind the gradient


@pytest.fixture(scope="module")
def contexts():
    """One context per (E, V): embed_grad_from_rows needs E, V and the staging array only, so the model around them is the smallest."""
    made = {}

    def get(E, V):
        if (E, V) not in made:
            made[(E, V)] = L.Context(E, 64, 64, V, max_B=2, max_T=1, lstm_dtype=F32)
        return made[(E, V)]

    yield get
    for ctx in made.values():
        ctx.close()


def from_rows(ctx, tok, x, V, E):
    """L.embed_grad_from_rows into the middle of a NaN buffer -> the gradient as [V][E] float32; lead-in and guard asserted untouched."""
    buf = torch.full((LEAD + V * E + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    rows = torch.as_tensor(np.array(x, dtype=np.float32, order="C")).cuda()   # a copy: the cases' arrays are read-only
    ids = torch.as_tensor(np.array(tok, dtype=np.int32)).cuda()
    L.embed_grad_from_rows(ctx, rows, ids, len(tok), buf[LEAD:LEAD + V * E])
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[:LEAD]).all(), "the lead-in before the gradient was written"
    assert np.isnan(h[LEAD + V * E:]).all(), "the guard behind V*E was written"
    return h[LEAD:LEAD + V * E].reshape(E, V).T   # memory [E][V]


def closeness(d, b):
    """The measured distances next to their derived bounds, for the log: the largest |d|, and the element that comes closest to its bound."""
    r = np.where(b > 0, d / np.where(b > 0, b, 1.0), 0.0)
    k = np.unravel_index(np.argmax(r), r.shape)
    return "max |d| %.3e; closest to its bound: |d| %.3e of %.3e (%.2e of the bound)" % (d.max(), d[k], b[k], r[k])


def assert_exact(got, ref, what):
    assert not np.isnan(got).any(), "%s: %d elements of the gradient were never written" % (what, int(np.isnan(got).sum()))
    bad = np.argwhere(got.astype(np.float64) != ref)
    assert bad.size == 0, "%s: %d elements differ, first (token, e) = %s: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], ref[tuple(bad[0])])


@pytest.mark.parametrize("c", er.CASES, ids=[c.id for c in er.CASES])
def test_ordered_sums_from_rows_match_the_float64_scatter(contexts, c):
    tok, x, ref = er.tokens(c), er.rows(c), er.reference(c)
    got = from_rows(contexts(c.E, c.V), tok, x, c.V, c.E)
    if c.kind == "int":
        assert_exact(got, ref, c.id)
        return
    assert not np.isnan(got).any()
    b = er.bound(tok, x, c.V)
    d = np.abs(got.astype(np.float64) - ref)
    print("%s: %s" % (c.id, closeness(d, b)))
    k = np.unravel_index(np.argmax(d - b), d.shape)
    assert (d <= b).all(), (c.id, k, d[k], b[k])


def test_staging_array_is_zero_again_after_every_call(contexts):
    E, V, n = 72, 301, 700
    ctx = contexts(E, V)
    rng = np.random.default_rng(5)
    sets = {"A": np.arange(0, V, 2), "B": np.arange(1, V, 2)}
    for name in ("A", "B", "A", "B"):
        tok = rng.choice(sets[name], size=n).astype(np.int32)
        x = rng.integers(-8, 9, size=(n, E)).astype(np.float32)
        ref = er.scatter_sum(tok, x, V)
        other = sets["B" if name == "A" else "A"]
        assert (ref[other] == 0).all()
        assert_exact(from_rows(ctx, tok, x, V, E), ref, "call with set %s" % name)


E, H, V, B, T, PDROP, SEED = 1000, 1000, 10640, 256, 11, 0.4, 0x5EED00000000D00D


@pytest.fixture(scope="module")
def production():
    """lossgradient at the benchmark's width with seeded dropout: per DETERMINISTIC setting, two exports of (rows, ids) and the dense
    grads[6] of a call without the export buffer."""
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=F32)
    param = L.initweights(ctx, seed=42)
    rng = np.random.default_rng(1)
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.01).astype(np.float32))
    pz = 1.0 / np.arange(1, V - 3 + 1)
    toks = (rng.choice(V - 3, size=(T, B), p=pz / pz.sum()) + 3).astype(np.int32)
    M = (T + 1) * B
    rows = torch.empty((M, E), device="cuda", dtype=torch.float32)
    ids = torch.empty((M,), device="cuda", dtype=torch.int32)
    out = {}
    for det in (0, 1):
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, det)
        L.set_embed_rows_buffer(ctx, rows, ids)
        exports = []
        for _ in range(2):
            rows.fill_(float("nan"))
            ids.fill_(-1)
            L.lossgradient(ctx, param, feats, toks, pdrop=PDROP, seed=SEED)
            torch.cuda.synchronize()
            exports.append((rows.cpu().numpy().copy(), ids.cpu().numpy().copy()))
        L.set_embed_rows_buffer(ctx, None, None)
        g, _ = L.lossgradient(ctx, param, feats, toks, pdrop=PDROP, seed=SEED)
        torch.cuda.synchronize()
        out[det] = (exports, L.from_jl(g[6]).copy())
    ctx.close()
    return toks, out


@pytest.mark.parametrize("det", [0, 1], ids=["atomics", "ordered"])
def test_lossgradient_embedding_gradient_is_the_sum_of_its_exported_rows(production, det):
    toks, out = production
    ((x, ids), (x2, ids2)), g = out[det]
    # the premise: f32 has no atomic split-K upstream of dXemb, so a second call computes the same rows
    assert np.array_equal(ids, ids2) and np.array_equal(x, x2), "two exports of the same call differ: the reference below would not be the call's"
    assert not np.isnan(x).any()
    assert np.array_equal(ids, np.vstack([np.full((1, B), L.BOS, np.int32), toks]).reshape(-1))   # [bos, tokens...], row m = s B + b
    cnt = np.bincount(ids, minlength=V)
    cnt[L.BOS] = 0   # step 0 feeds bos to every row; the Zipf claim is about the words
    assert cnt.max() > 200, "the busiest word owns %d rows: not the Zipf case this test claims to be" % cnt.max()
    ref, b = er.scatter_sum(ids, x, V), er.bound(ids, x, V, extra=1)
    assert g.shape == (V, E) and not np.isnan(g).any()
    d = np.abs(g.astype(np.float64) - ref)
    print("DETERMINISTIC = %d: busiest word %d rows; max |ref| %.3e; %s" % (det, cnt.max(), np.abs(ref).max(), closeness(d, b)))
    k = np.unravel_index(np.argmax(d - b), d.shape)
    assert (ref[b == 0] == 0).all() and (d <= b).all(), (k, d[k], b[k])


def test_exported_rows_carry_the_seeded_mask_and_its_kept_share_is_unbiased(production):
    _, out = production
    x = out[1][0][0][0]
    mask = dr.masks(SEED, PDROP, T, B, E, H)[0].reshape((T + 1) * B, E)   # row m = s B + b, as exported
    dropped = mask == 0
    assert (x[dropped] == 0).all(), "%d exported elements are non-zero where the host mask drops" % int((x[dropped] != 0).sum())
    zeros_kept = float((x[~dropped] == 0).mean())
    n, q = x.size, 1.0 - PDROP
    share = float((x != 0).mean())
    print("exported rows: %.4f non-zero (host mask keeps %.4f); %.2e of the kept elements are zero" % (share, float((~dropped).mean()), zeros_kept))
    assert zeros_kept < 1e-3
    # on the device: the share of elements that pass, within 4 binomial standard deviations of 1 - p (and the 0.1 % of kept zeros above)
    assert -4 * np.sqrt(PDROP * q / n) - 1e-3 <= share - q <= 4 * np.sqrt(PDROP * q / n), share
