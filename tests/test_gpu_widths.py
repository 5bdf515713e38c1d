"""GPU: the LSTM stack at the width sets of tests/width_cases.py -- hidden and embedding widths off the multiple-of-4 grid, under 16, above 1024,
and H1 != H2 -- where until now only E = H multiples of 4 up to 1024 ran in bf16.  tests/test_width_cases.py (CPU) holds the table's
properties, the references at these widths and the decodes' tie margins.

No tolerance is new.  Each case takes the bound of the existing test of the same route:
  bf16 loss / gradients   parity_util.assert_bf16_matches_emulation against emulated_reference (which carries the plain f32 oracle's bound too)
  f32 loss / gradients    test_backward_glue_shapes_vs_oracle_fp32: loss 1e-5 relative, gradients rtol 1e-3 + atol 1e-5
  route against route     test_fused_recurrence_small_batch_forms_equal_ring_forms: loss 1e-4, gradients 1e-2 in norm
  decodes                 f32 test_wide_beam_f32_equals_oracle; bf16 test_bf16_single_step_and_beam_search_vs_emulating_oracle and
                          test_gpu_decode_epilogue.compare; scores test_gpu_score.py; samples test_gpu_sample.replay
  update                  test_gpu_fused_update.py, test_adam_trajectory_vs_golden
  activity                test_gpu_activity._f32_assert / _bf16_assert, test_gpu_activity_dropout._f32_close / _bf16_close
T = 3 (S = 4 steps: the step kernels run for s = 1 .. 3) and only the row counts that select a route.
"""
import functools

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import activity as A
from lrcn_amd import lrcn as L
from oracle import oracle as orc
from parity_util import assert_bf16_matches_emulation, emulated_reference

import varlen_ref as vr
import width_cases as wc
from activity_drop_ref import emulated_drop, reference_drop, seeded_masks
from test_gpu_activity import _bf16_assert, _f32_assert
from test_gpu_activity_dropout import _bf16_close, _f32_close
from test_gpu_decode_epilogue import compare as compare_decodes
from test_gpu_sample import replay as sample_replay
from test_gpu_score import captions_of, oracle_scores

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
T = 3
# Row counts per set: 21 (one partial 32-row block: lstm_rec_fwd2_kernel<8> + lstm_rec_bwd_kernel<1, 8> with a 5-row second block; over1024:
# lstm_rec_fwd_kernel<2>), 40 (two 32-row blocks with a tail forward, 16-row blocks with a tail of 8 backward; over1024: lstm_rec_fwd_kernel<4>),
# 130 (above kLstmFusedMaxRows: GEMM + cell kernel; over1024: the recurrent and Wproj GEMMs at K = 1041 / 1042, transposes with shift = 130).
ROWS = (21, 40, 130)


def ctx_for(name, B, dtype, V=None, det=False, max_T=T, beside=0):
    E, H1, H2, V0, nl = wc.CAPTION[name]
    kw = dict(vgg_dtype=BF16, max_images=1) if beside else {}
    ctx = L.Context(E, H1, H2, V or V0, max_B=B, max_T=max_T, lstm_dtype=dtype, n_layers=nl, **kw)
    if det:
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    if beside:   # what dp.py sets up: VGG weights loaded and the convolution grids capped -> the LSTM step is "beside the convolutions"
        L.vgg_load(ctx, *vgg_weights())
        L.vgg_set_wg_cap(ctx, beside)
    return ctx


@functools.lru_cache(maxsize=None)
def vgg_weights():
    return L.synthetic_vgg_weights(seed=1)


@functools.lru_cache(maxsize=None)
def reference(name, B, masks=False):
    """(emulated loss, emulated gradients with .f32 = (loss, gradients) of the plain oracle), once per process and never written to."""
    c = wc.batch(name, B, T, masks)
    return emulated_reference(wc.model(name), c.feats, c.tokens, mask1=c.mask1, mask2=c.mask2)


def lossgrad(ctx, name, B, masks=False):
    c = wc.batch(name, B, T, masks)
    grads, val = L.lossgradient(ctx, L.model_from_arrays(wc.model(name).p), L.to_jl(c.feats), c.tokens, mask1=c.mask1, mask2=c.mask2)
    torch.cuda.synchronize()
    return val, [L.from_jl(g).astype(np.float64) for g in grads]


def assert_f32(val, grads, ref, what):
    ref_loss, ref_g = ref[1].f32
    assert abs(val - ref_loss) <= 1e-5 * abs(ref_loss), (what, val, ref_loss)
    for n, g in zip(orc.PARAM_NAMES, grads):
        if ref_g.p[n].size:
            np.testing.assert_allclose(g, ref_g.p[n], rtol=1e-3, atol=1e-5, err_msg="%s %s" % (what, n))


def assert_routes_agree(a, b, scale, what):
    assert abs(a[0] - b[0]) <= 1e-4 * abs(scale), (what, a[0], b[0])
    for n, x, y in zip(orc.PARAM_NAMES, a[1], b[1]):
        assert np.linalg.norm(x - y) <= 1e-2 * np.linalg.norm(y) + 1e-12, (what, n)


# ---------------------------------------------------------------------------------------------- a. loss and gradients, every width set
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(wc.CAPTION))
def test_loss_and_gradients_at_every_width_set(name, dtype, monkeypatch):
    """Every set of width_cases.CAPTION at 21, 40 and 130 rows, against the oracle.
    All dtypes: prepare_weights_kernel's scalar branches (`vec` false at H % 4 != 0, and at E % 4 != 0 through `cs`: the element-wise direct
    and transposed copies), transpose_multi_kernel's vin / vout false (ld_src = H or E off 4, shift = B = 21), embed_stage_to_grad_kernel's
    scalar stores (every V here is off 4).
    bf16, the last-workgroup unit masks of lstm_rec_fwd2_kernel<8> and lstm_rec_bwd_kernel<1, 8>: 1 valid unit (res1: H1 = 17), 2 (res1:
    H2 = 18), 3 (res3: 19), 4 (edge68, eodd), 5 (res5: 21), 6 (res3: H2 = 22) and 7 (res7: 23).  under16 (15, 14) and min (1, 2) are below
    lstm_fused_eligible's 16 and run GEMM + cell kernel at every batch.  over1024: 17 K-tiles, so launch_lstm_rec_fwd refuses the 8-unit
    form and lstm_rec_fwd_kernel<2> / <4> (16 units, one valid in the last workgroup) pair with lstm_rec_bwd_kernel<1, 8>.
    uneq_a / uneq_b: H1 != H2 alone.  *_1f: X1 = E + H / 2 (62, 1558).
    bf16 also runs 21 and 40 rows under LRCN_LSTM_REC2=0 (the 16-unit ring forms <2> and <4>, forward and backward) and 21 rows under
    LRCN_LSTM_FUSED=0 (the GEMM + cell fallback at small batch)."""
    for B in ROWS:
        ref = reference(name, B)
        ctx = ctx_for(name, B, dtype)
        what = "%s B=%d" % (name, B)
        got = lossgrad(ctx, name, B)
        if dtype == F32:
            assert_f32(*got, ref, what)
        else:
            assert_bf16_matches_emulation(*got, *ref, what)
            for knob, value in (("LRCN_LSTM_REC2", "0"), ("LRCN_LSTM_FUSED", "0")):
                if B > 40 or (knob == "LRCN_LSTM_FUSED" and B != 21):
                    continue
                monkeypatch.setenv(knob, value)
                other = lossgrad(ctx, name, B)
                monkeypatch.delenv(knob)
                assert_bf16_matches_emulation(*other, *ref, "%s %s=%s" % (what, knob, value))
                assert_routes_agree(got, other, ref[0], "%s %s=%s" % (what, knob, value))
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["res2", "res2_1f"])
def test_explicit_dropout_masks_at_odd_widths(name, dtype):
    """res2 (E = 37, H2 = 46, h = 23) and its one-layer form (E + h = 62) with explicit multipliers on both dropout sites: concat_x2's and
    dx2_mask_reduce_kernel's columns nl = nr = 23, the embedding multipliers at odd E (embed gather forward, the scatter backward)."""
    for B in (21, 130):
        ref = reference(name, B, True)
        ctx = ctx_for(name, B, dtype)
        got = lossgrad(ctx, name, B, True)
        if dtype == F32:
            assert_f32(*got, ref, "%s masks B=%d" % (name, B))
        else:
            assert_bf16_matches_emulation(*got, *ref, "%s masks B=%d" % (name, B))
        ctx.close()


# ---------------------------------------------------------------------------------------------- b. beside the convolutions
@pytest.mark.parametrize("name", ["res1", "res3", "over1024"])
def test_twelve_unit_forms_beside_the_convolutions_at_odd_widths(name, monkeypatch):
    """As test_twelve_unit_recurrence_forms_beside_the_vgg_forward: VGG weights loaded, grids capped at 160, 21 rows.  lstm_rec_fwd2_kernel<12>
    and lstm_rec_bwd_kernel<2, 12> with 5 (res1: 17 % 12), 7 (res3: 19 % 12; the half piece of rows 8 .. 11 then holds no valid row) and 9
    (over1024: 1041 % 12) valid units in the last workgroup; over1024's 17 K-tiles make launch_lstm_rec_fwd refuse the 12-unit forward
    (R2_KT = 16) while launch_lstm_rec_bwd keeps the 12-unit backward.  LRCN_LSTM_REC3=0: the 16-unit ring forms."""
    B = 21
    ref = reference(name, B)
    res = {}
    for knob in ("32", "0"):
        monkeypatch.setenv("LRCN_LSTM_REC3", knob)
        ctx = ctx_for(name, B, BF16, beside=160)
        for _ in range(2):   # twice: scratch buffers carry the first call's values
            res[knob] = lossgrad(ctx, name, B)
        ctx.close()
        assert_bf16_matches_emulation(*res[knob], *ref, "%s beside, LRCN_LSTM_REC3=%s" % (name, knob))
    assert_routes_agree(res["32"], res["0"], ref[0], name)


@pytest.mark.parametrize("B", [256, 300])
def test_rows_of_the_beside_window_at_a_width_off_the_vector_grid(B):
    """mid_odd (H1 = 203, H2 = 206) at 256 and 300 rows beside the capped convolution grids: the "bg" dispatch of the recurrent GEMMs (256 x 128
    tiles) with N = 4 H = 812 / 824 and K = 203 / 206, row-block tail of 44 rows, cell kernels at H % 4 != 0."""
    ref = reference("mid_odd", B)
    ctx = ctx_for("mid_odd", B, BF16, beside=224)
    assert_bf16_matches_emulation(*lossgrad(ctx, "mid_odd", B), *ref, "mid_odd beside B=%d" % B)
    ctx.close()


# ---------------------------------------------------------------------------------------------- c. guards refuse
def as_bytes(res):
    return [np.float64(res[0]).tobytes()] + [g.tobytes() for g in res[1]]


def test_cell_epilogue_knob_is_refused_off_the_vector_grid(monkeypatch):
    """lstm_epi_on carries !(H1 & 3) && !(H2 & 3): on mid_odd at 256 rows beside the convolutions (where an H on the grid takes the cell-epilogue
    route, test_cell_epilogue_training_route_partial_tiles_vs_oracle) LRCN_LSTM_EPI=1 and =f must not change one bit of the loss or of the
    nine gradients of a deterministic context."""
    B = 256
    ctx = ctx_for("mid_odd", B, BF16, det=True, beside=224)
    base = lossgrad(ctx, "mid_odd", B)
    assert_bf16_matches_emulation(*base, *reference("mid_odd", B), "mid_odd, ordered sums")
    for knob in ("1", "f"):
        monkeypatch.setenv("LRCN_LSTM_EPI", knob)
        assert as_bytes(lossgrad(ctx, "mid_odd", B)) == as_bytes(base), "LRCN_LSTM_EPI=%s changed the result at H %% 4 != 0" % knob
    ctx.close()


@pytest.mark.parametrize("knob", ["1", "f"])
def test_cell_epilogue_training_route_at_an_embedding_width_off_the_grid(knob, monkeypatch):
    """eodd (E = 37, H1 = H2 = 68) at 256 rows beside the convolutions with LRCN_LSTM_EPI=1 / =f: lstm_epi_on accepts (it looks at H1 and H2
    only), and the gate-interleaved recurrent copy (giH = 68) is written by prepare_weights_kernel from W1's memory image with C = 37 + 68 and
    cs = 37: `vec` false, a quad of columns straddles the split.  Against the emulating oracle, as
    test_cell_epilogue_training_route_partial_tiles_vs_oracle (H = 68 < 128: the backward epilogue is skipped, =1 runs as =f)."""
    B = 256
    ctx = ctx_for("eodd", B, BF16, beside=224)
    monkeypatch.setenv("LRCN_LSTM_EPI", knob)
    assert_bf16_matches_emulation(*lossgrad(ctx, "eodd", B), *reference("eodd", B), "eodd, LRCN_LSTM_EPI=%s" % knob)
    ctx.close()


def route_predicates(name, V):
    """decode.hip's predicates at 256 rows and more, restated: (decode_epi_on, decode_tables_on, smax_records_on)."""
    _, H1, H2, _, nl = wc.CAPTION[name]
    epi = not (H1 & 3) and not (H2 & 3)
    return {"LRCN_DECODE_EPI": epi, "LRCN_DECODE_TABLES": epi and nl == 2 and H1 > 64 and H2 > 64,
            "LRCN_DECODE_SMAX": epi and V >= 256 and not (V & 3) and H2 > 64, "LRCN_SCORE_FUSED": V >= 256 and not (V & 3) and H2 > 64}


def oracle_beam(m, f, K):
    with orc.emulate_bf16():
        t, p = orc.beam_search(m, f, K, wc.NWORD)
    return list(t), p


@pytest.mark.parametrize("key", list(wc.DECODE_ROUTES))
def test_decode_route_knobs_at_the_guards(key, monkeypatch):
    """Batched beam decode of 52 images x 5 hypotheses = 260 rows.  mid_odd (H % 4 != 0, V = 301 and 300): decode_epi_on refuses, and with it
    tables and records; eodd (E = 37, H = 68, V = 300): all three accept, and the concatenated weights are made by prepare_weights_kernel's
    scalar branch with permuted destination rows (permH = 68, C = 37 + 68 = 105, cs = 37), decode_prep_kernel copies 37 = 4 x 8 + 5 elements;
    edge64 (H = 64): the cell epilogue runs, decode_tables_on (H1 > 64 && H2 > 64) and smax_records_on (H2 > 64) refuse; edge68 at
    V = 300: all three accept (and 68 % 8 = 4 leaves decode_prep_kernel's and decode_prep_h_kernel's copies a scalar tail of four elements, the
    former under LRCN_DECODE_TABLES=0); V = 302 and 301: smax_records_on refuses on V & 3.  Where the predicate refuses, LRCN_x=0 against unset is the
    same decode bit for bit; where it accepts, test_gpu_decode_epilogue.compare.  Either way the decode agrees with the emulating oracle."""
    d = wc.DECODES["route-" + key]
    m = wc.decode_model(d.name, d.V)
    feats = wc.decode_feats(d.N)
    ctx = ctx_for(d.name, d.N * d.K, BF16, V=d.V, max_T=2)
    param = L.model_from_arrays(m.p)
    base = L.beam_search_batch(ctx, param, L.to_jl(feats), d.K, wc.NWORD)
    accepts = route_predicates(d.name, d.V)
    for knob in ("LRCN_DECODE_EPI", "LRCN_DECODE_TABLES", "LRCN_DECODE_SMAX"):
        monkeypatch.setenv(knob, "0")
        off = L.beam_search_batch(ctx, param, L.to_jl(feats), d.K, wc.NWORD)
        monkeypatch.delenv(knob)
        if accepts[knob]:
            compare_decodes(base, off, d.N)
        else:
            assert [t for t, _ in off] == [t for t, _ in base], "%s=0 changed a decode it has no say in" % knob
            assert np.asarray([p for _, p in off], np.float32).tobytes() == np.asarray([p for _, p in base], np.float32).tobytes(), knob
    picks = [0, 1, d.N // 2, d.N - 2, d.N - 1]
    agree = 0
    for i in picks:
        rt, rp = oracle_beam(m, feats[i], d.K)
        if base[i][0] == rt:
            agree += 1
            assert abs(base[i][1] - rp) <= 5e-2 * abs(rp) + 1e-30, (i, base[i][1], rp)
    assert agree >= len(picks) - 1, agree
    ctx.close()


@pytest.mark.parametrize("key", list(wc.DECODE_ROUTES))
def test_score_route_knob_at_the_guards(key, monkeypatch):
    """score_matrix of 8 images x 33 captions = one piece of 264 pair rows: score_fused_on = smax_records_on, which has no H & 3 term.  Refused
    (mid_odd at V = 301, edge64, V = 302, V = 301): LRCN_SCORE_FUSED=0 gives the same float scores bit for bit; accepted (edge68 and eodd at
    V = 300, and mid_odd at V = 300: the records epilogue at H2 = 206, K = 256 with 50 columns of padding): test_fused_and_unfused_routes_agree's
    1e-3 per step.  Both against the emulating oracle by test_bf16_production_matches_emulating_oracle's bound."""
    name, V = wc.DECODE_ROUTES[key]
    m = wc.decode_model(name, V)
    N, M = 8, 33
    feats = wc.decode_feats(N)
    caps = captions_of(M, V, 5, lens=np.random.default_rng(M).integers(1, 7, size=M))
    ctx = ctx_for(name, N * M, BF16, V=V, max_T=2)
    param = L.model_from_arrays(m.p)
    a = L.score_matrix(ctx, param, L.to_jl(feats), caps)
    monkeypatch.setenv("LRCN_SCORE_FUSED", "0")
    b = L.score_matrix(ctx, param, L.to_jl(feats), caps)
    ctx.close()
    if route_predicates(name, V)["LRCN_SCORE_FUSED"]:
        steps = np.array([len(c) + 1 for c in caps], np.float64)[None, :]
        assert (np.abs(a - b) / steps <= 1e-3).all(), (np.abs(a - b) / steps).max()
    else:
        assert np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()
    pairs = [(n, c) for n in (0, N - 1) for c in range(M)]
    for (n, c), v in oracle_scores(m, feats, caps, pairs, bf16=True).items():
        assert abs(a[n, c] - v) <= 5e-2 + 2e-2 * abs(v), (n, c, a[n, c], v)


# ---------------------------------------------------------------------------------------------- d. update and shadows
UPDATE_B, UPDATE_STEPS, update_batches = wc.UPDATE_B, wc.UPDATE_STEPS, wc.update_batches


def trajectory(name, dtype, fused, gclip=0.0):
    """UPDATE_STEPS train_steps on a deterministic context: losses, [parameters + m + v] and the nine gradients after every step, the clip
    counters."""
    ctx = ctx_for(name, UPDATE_B, dtype, det=True)
    ctx.set_option(_lib.LRCN_OPT_FUSED_UPDATE, 1 if fused else 0)
    param = L.model_from_arrays(wc.model(name).p)
    optim = L.initparams(param)
    grads = L.zeros_like_model(param)
    losses, states, gs = [], [], []
    for feats, toks in update_batches(name):
        losses.append(L.train_step(ctx, param, optim, grads, L.to_jl(feats), toks, pdrop=0.0, want_loss=True, gclip=gclip))
        torch.cuda.synchronize()
        states.append([L.from_jl(t).copy() for t in list(param) + list(optim.m) + list(optim.v)])
        gs.append([L.from_jl(t).copy() for t in grads])
    st = L.clip_stats(ctx) if gclip else None
    ctx.close()
    return np.array(losses), states, gs, st


@pytest.mark.parametrize("name,gclip", [("res2", 0.0), ("res3", 0.0), ("over1024", 0.0), ("res2_1f", 0.0), ("res2", 1e-3), ("over1024", 1e-3)])
def test_fused_update_at_odd_widths(name, gclip):
    """LRCN_OPT_FUSED_UPDATE on against off, bf16: prepare_weights_kernel<T, true> (and <T, true, true> with gclip = 1e-3, far below any norm
    here: every step clips) makes the next step's shadows in its scalar branches -- res2: C = E + H1 = 87 with cs = 37, res3: C = 54 / cs =
    35, over1024: C = 2078 / cs = 1037, res2_1f: C = 112 with the split of the [embedding | x_cnn | h] rows.  The first step is bit-identical
    outside Wembed (test_first_fused_step_equals_unfused_exactly), the trajectory follows by test_gpu_fused_update.py's bounds.  The clipped
    form runs on res2 and over1024 only (the same kernel; two widths are enough)."""
    la, sa_all, _, sa = trajectory(name, BF16, False, gclip)
    lb, sb_all, _, sb = trajectory(name, BF16, True, gclip)
    (a1, a3), (b1, b3) = (sa_all[0], sa_all[-1]), (sb_all[0], sb_all[-1])
    assert np.all(np.isfinite(la)) and la[-1] != la[0]
    for k, (a, b) in enumerate(zip(a1, b1)):
        if k % 9 == 6:
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-7)
        else:
            assert np.array_equal(a, b), (k, orc.PARAM_NAMES[k % 9])
    np.testing.assert_allclose(la, lb, rtol=1e-6)
    for k, (a, b) in enumerate(zip(a3, b3)):
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6, err_msg=str(k))
    if gclip:
        assert sa["clipped"] == sb["clipped"] == UPDATE_STEPS and sa["skipped"] == sb["skipped"] == 0, (sa, sb)


@pytest.mark.parametrize("name", wc.ADAM_SETS)
def test_unfused_trajectory_follows_the_oracle_adam_f32(name):
    """train_step in f32 (lossgradient + adam_kernel) for three steps against orc.adam on the oracle's own gradients
    (width_cases.adam_reference).  Every step's loss within 2e-5 and the final parameters within 5e-6, test_adam_trajectory_vs_golden's
    bounds, on every element that adam_reference finds well conditioned (all but 143 of 141074 for res2, 19 of 59263 for res3, 99380 of
    20.2 M for over1024, 72 of 136528 for res2_1f: tests/test_width_cases.py holds those counts and shows that the oracle's own float build
    keeps 5e-6 exactly there); the ill-conditioned ones, whose gradients are float32 noise that Adam divides by sqrt(v), within
    adam_reference's .bound (5e-6 plus five times its measured allowance).  Measured: the worst well-conditioned element 4.2e-6
    (over1024 W1), 2.8e-7 elsewhere; the worst ill-conditioned one 2.2e-5.  The first step's nine gradients, taken at identical parameters,
    also meet the oracle's by test_backward_glue_shapes_vs_oracle_fp32's bounds."""
    losses, states, gs, _ = trajectory(name, F32, False)
    ref = wc.adam_reference(name)
    for t in range(UPDATE_STEPS):
        assert abs(losses[t] - ref.losses[t]) <= 2e-5 * abs(ref.losses[t]), (t, losses[t], ref.losses[t])
    for k, n in enumerate(orc.PARAM_NAMES):
        if n not in ref.params:
            continue
        d = np.abs(states[-1][k].astype(np.float64) - ref.params[n])
        ok, ill = ~ref.ill[n], ref.ill[n]
        print("%s %s: worst well-conditioned %.2e, worst ill-conditioned %.2e (%d elements)" % (
            name, n, d[ok].max(), d[ill].max() if ill.any() else 0.0, int(ill.sum())))
        assert (d[ok] <= wc.ADAM_ATOL).all(), "%s: %d well-conditioned elements past %g, worst %.3e" % (
            n, int((d[ok] > wc.ADAM_ATOL).sum()), wc.ADAM_ATOL, d[ok].max())
        assert (d <= ref.bound[n]).all(), "%s: worst %.3e at a bound of %.3e" % (n, d.max(), ref.bound[n].ravel()[d.argmax()])
    # the gradients of step 1 are taken at identical parameters; later steps' parameters differ from the oracle's by what is bounded above
    m = wc.model(name)
    feats, toks = update_batches(name)[0]
    _, g = orc.loss(m, feats, toks, want_grad=True)
    for k, n in enumerate(orc.PARAM_NAMES):
        if n in ref.params:
            np.testing.assert_allclose(gs[0][k], g.p[n], rtol=1e-3, atol=1e-5, err_msg="step 1 gradient %s" % n)


# ---------------------------------------------------------------------------------------------- e. ordered embedding sums, mixed lengths
@functools.lru_cache(maxsize=None)
def varlen_case(name):
    B = 5 if name == "over1024" else 24   # (the row-by-row oracle needs a second per row above 1024)
    c = wc.batch(name, B, T)
    lens = np.random.default_rng(B).choice([0, 1, T], size=B).astype(np.int32)
    lens[:3] = (T, 0, 1)
    # a "global" token count that is a multiple of every len + 1 (1, 2, 4): the emulating oracle then rounds d(logits) at the library's scale
    nt = vr.norm_tokens_of(lens)
    nt += -nt % 4
    ref = vr.emulated_reference(wc.model(name), c.feats, c.tokens, lens, nt, row_norms=vr.integer_row_norms(lens, nt))
    return c, lens, nt, ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["res2", "over1024"])
def test_ordered_embedding_sums_and_mixed_lengths_at_odd_E(name, dtype):
    """LRCN_OPT_DETERMINISTIC and the variable-length entry: embed_segsum_kernel's `e0 + k < E` tail at E % 4 = 1 -- res2: E = 37, the last
    float4 lane holds one column; over1024: E = 1037, five column slices of 256 with 13 columns in the last -- and embed_stage_to_grad_kernel
    at V % 4 != 0.  Every row starts with bos, so its segment has B rows and all eight waves of a workgroup add.  Against tests/varlen_ref.py
    (f32: test_mixed_lengths_f32_vs_oracle's bounds; bf16: the emulating oracle), and the call repeats itself bit for bit."""
    c, lens, nt, (e_loss, e_g) = varlen_case(name)
    ctx = ctx_for(name, c.B, dtype, det=True)
    param = L.model_from_arrays(wc.model(name).p)
    out = []
    for _ in range(2):
        g, val = L.lossgradient(ctx, param, L.to_jl(c.feats), c.tokens, lens=lens, norm_tokens=nt)
        torch.cuda.synchronize()
        out.append((val, [L.from_jl(x).astype(np.float64) for x in g]))
    ctx.close()
    assert as_bytes(out[0]) == as_bytes(out[1])
    if dtype == F32:
        f_loss, f_g = e_g.f32
        assert abs(out[0][0] - f_loss) <= 1e-5 * abs(f_loss), (out[0][0], f_loss)
        for n, g in zip(orc.PARAM_NAMES, out[0][1]):
            np.testing.assert_allclose(g, f_g.p[n], rtol=1e-3, atol=1e-5, err_msg=n)
    else:
        assert_bf16_matches_emulation(*out[0], e_loss, e_g, "%s mixed lengths, ordered sums" % name)


# ---------------------------------------------------------------------------------------------- f. decodes under 256 rows
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("key", list(wc.DECODE_SMALL))
def test_beam_search_under_256_rows_at_odd_widths(key, dtype):
    """beam_search_batch and the single-image beam_search, 5 images, against orc.beam_search: the embedding gather, the state gather by parent and
    the step's GEMMs at K = E + H1 and 2 H2 off the grid (res1, res2), under 16 (under16), at the smallest model (min: V = 3,
    K = 2) and at 17 K-tiles (over1024).  f32 as test_wide_beam_f32_equals_oracle: the oracle's tokens, probability to 1e-4 (the CPU file
    asserts that no winner is tied).  bf16 as test_bf16_single_step_and_beam_search_vs_emulating_oracle: at most one image of five may fall
    the other way, probabilities to 5e-2."""
    d = wc.DECODES[key]
    m = wc.decode_model(d.name, d.V)
    feats = wc.decode_feats(d.N)
    ctx = ctx_for(d.name, max(d.N * d.K, 4), dtype, max_T=2)
    param = L.model_from_arrays(m.p)
    batch = L.beam_search_batch(ctx, param, L.to_jl(feats), d.K, wc.NWORD)
    same = {"per image": 0, "batched": 0}
    for i in range(d.N):
        one = L.beam_search(ctx, param, L.to_jl(feats[i:i + 1]), d.K, wc.NWORD)
        if dtype == F32:
            rt, rp = orc.beam_search(m, feats[i], d.K, wc.NWORD)
            rt = list(rt)
        else:
            rt, rp = oracle_beam(m, feats[i], d.K)
        for label, (t, p) in (("per image", one), ("batched", batch[i])):
            if dtype == F32:
                assert t == rt, (label, i, t, rt)
                assert abs(p - rp) <= 1e-4 * abs(rp), (label, i, p, rp)
            elif t == rt:
                same[label] += 1
                assert abs(p - rp) <= 5e-2 * abs(rp) + 1e-30, (label, i, p, rp)
    ctx.close()
    if dtype == BF16:
        assert min(same.values()) >= d.N - 1, same


def test_seeded_samples_replay_at_odd_widths():
    """sample_batch on res2 in f32, temperature 0.7 and top_k 3, replayed through the oracle's logits by test_gpu_sample.replay: every drawn
    token is the host's argmax of z / T + g over the admitted columns and the log-likelihood is the host's."""
    m = wc.decode_model("res2")
    N, S, seed = 5, 4, 0x1234567890ABCDEF
    feats = wc.decode_feats(N)
    ctx = ctx_for("res2", N * S, F32, max_T=2)
    res = L.sample_batch(ctx, L.model_from_arrays(m.p), L.to_jl(feats), S, wc.NWORD, temperature=0.7, top_k=3, seed=seed)
    ctx.close()
    exact, steps = sample_replay(m, feats, res, S, 0.7, 3, seed, list(range(N * S)), bf16=False)
    assert exact == steps, (exact, steps)


def test_score_matrix_at_odd_widths_f32():
    """score_matrix on res2 in f32 against the oracle's per-step log-softmax (test_f32_matrix_matches_oracle's bound): k_score_prep and the
    per-token / per-image tables at E = 37, H1 = 50, H2 = 46, h = 23."""
    m = wc.decode_model("res2")
    N, M = 5, 11
    feats = wc.decode_feats(N)
    caps = captions_of(M, m.V, 5, lens=np.array([5, 1, 8, 3, 2, 8, 7, 1, 4, 6, 2]))
    ctx = ctx_for("res2", 64, F32, max_T=2)
    s = L.score_matrix(ctx, L.model_from_arrays(m.p), L.to_jl(feats), caps)
    ctx.close()
    for (n, c), v in oracle_scores(m, feats, caps, [(n, c) for n in range(N) for c in range(M)]).items():
        assert abs(s[n, c] - v) <= 1e-5 * (1 + abs(v)), (n, c, s[n, c], v)


# ---------------------------------------------------------------------------------------------- g. activity
ACT_T = 4


def activity_model(shape, B, dtype):
    F, H, C_ = shape
    m = A.ActivityModel(F, H, C_, max_B=B, max_T=ACT_T, dtype=dtype, seed=7)
    return (m,) + wc.activity_inputs(F, H, C_, ACT_T, B)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", wc.ACTIVITY, ids=["F%d-H%d-C%d" % s for s in wc.ACTIVITY])
def test_activity_at_odd_widths(shape, dtype):
    """lrcn_act_loss_grad and lrcn_act_predict at width_cases.ACTIVITY with mixed lengths that include 1 and T, against tests/activity_ref.py by
    test_gpu_activity.py's own comparisons.  3 and 40 rows (bf16: the fused step kernels' unit masks at H = 50, 17, 1041 -- 2, 1, 1 valid
    units of 8; H = 15 and 1: GEMM + cell kernel), and for H = 17 and H = 1041 also 130 rows, above the fused limit: the recurrent GEMM and
    the cell kernels at N = 4 H = 68 / 4164, K = 17 / 1041."""
    F, H, C_ = shape
    for B in (3, 40) + ((130,) if H in (17, 1041) else ()):
        m, x, lab, lens = activity_model(shape, B, dtype)
        if dtype == F32:
            _f32_assert(m, x, lab, lens, ACT_T, B, "f32 %s B=%d" % (shape, B))
        else:
            _bf16_assert(m, x, lab, lens, ACT_T, B)
        m.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_activity_seeded_dropout_at_odd_widths(dtype):
    """(F, H, C) = (33, 17, 5) with seeded dropout on the frame features and the LSTM output, 40 rows: act_frames_kernel<T, true> at F % 4 = 1
    and the output mask at H = 17, through test_gpu_activity_dropout.py's references and bounds."""
    F, H, C_ = shape = wc.ACTIVITY[1]
    B, p_in, p_out, seed = 40, 0.5, 0.5, 4242
    m, x, lab, lens = activity_model(shape, B, dtype)
    if dtype == BF16:
        x = (x * np.sqrt(1.0 - p_in)).astype(np.float32)   # as test_bf16_parity_with_the_rounding_emulation: masked features of unit variance
    mi, mo = seeded_masks(seed, p_in, p_out, ACT_T, B, F, H)
    loss = m.loss_grad(x, lab, lens, ACT_T, pdrop_in=p_in, pdrop_out=p_out, drop_seed=seed)
    g = [L.from_jl(t).astype(np.float64) for t in m.grads]
    P = [L.from_jl(p).astype(np.float64) for p in m.params]
    m.close()
    if dtype == F32:
        rl, rg = reference_drop(*P, x, lab, lens, ACT_T, B, mi, mo)
        assert abs(loss - rl) <= 1e-4 * abs(rl), (loss, rl)
        _f32_close(g, rg, "f32 %s" % (shape,))
    else:
        el, eg = emulated_drop(*P, x, lab, lens, ACT_T, B, mi, mo, bf16=True)
        _bf16_close(loss, g, el, eg)
