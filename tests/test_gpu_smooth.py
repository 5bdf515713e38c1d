"""GPU: label smoothing in the caption loss kernels (include/lrcn_smooth.h) against tests/smooth_ref.py, the float64 restatement that
tests/test_smooth_ref.py holds to torch's cross_entropy(label_smoothing=).

1. the kernels alone through lrcn_xent_logits, on both sides of every rung of the register ladder and in the streaming form;
2. smooth == 0 returns the bits of the calls without it;  3. the whole model in f32;  4. in bf16;  5. with scheduled sampling;
6. the training step and the trainer;  7. argument checks.

Bounds.  f32 row terms and losses: 1e-5 relative, the project's f32 loss bound.  f32 d(logits): 1e-5 |ref| + 2e-6 |row scale| per element
-- ten times the 2e-7 a float32 restatement of the kernel's order showed on the host, the margin being for the device's expf and its
summation order.  Every active row's d(logits) sums to 0 within 1e-5 |row scale| (the target distribution sums to 1).  bf16 d(logits): the
bf16 rounding of the float64 reference within one bf16 ulp plus the f32 bound.  f32 gradients: rtol 1e-3 + atol 1e-5; bf16 model: 2e-2 on
the loss and per tensor in norm (tests/parity_util.py)."""
import ctypes as C
import functools
import os
import socket

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib, dp
from lrcn_amd import lrcn as L
from oracle import oracle as orc
from parity_util import assert_bf16_near_f32_oracle

import sched_ref as sr
import smooth_ref as smr
import varlen_ref as vr
import xent_ladder_cases as xl

pytestmark = pytest.mark.gpu
F32, BF16 = lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16
NAMES = ("lrcn_loss_smooth", "lrcn_loss_grad_smooth", "lrcn_train_step_smooth", "lrcn_smooth_stats", "lrcn_xent_logits")
EPS = float(np.float32(0.1))   # the float the library receives for 0.1
ALWAYS = 1e-3                  # tests/test_gpu_clip.py's: far below any gradient norm met here, every step clips


def make(seed, B, T, E, H, V, dtype, n_layers=2, det=False):
    rng = np.random.default_rng(seed)
    m = orc.init_weights(E, H, H, V, seed=seed + 1, n_layers=n_layers)
    feats = (rng.standard_normal((B, 4096)) * 0.02).astype(np.float32)
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    ctx = L.Context(E, H, H, V, max_B=B, max_T=max(T, 1), lstm_dtype=dtype, n_layers=n_layers)
    if det:
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    return rng, m, feats, tokens, ctx, L.model_from_arrays(m.p)


def host(grads):
    return [L.from_jl(g).copy() for g in grads]


def grads_close_f32(got, ref_g, what=""):
    for n, g in zip(orc.PARAM_NAMES, got):
        if ref_g.p[n].size:
            np.testing.assert_allclose(g if isinstance(g, np.ndarray) else L.from_jl(g), ref_g.p[n], rtol=1e-3, atol=1e-5, err_msg="%s %s" % (what, n))


def same_bits(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), "%s: tensor %d differs" % (what, k)


def mixed_case(rng, B, T):
    """tests/test_gpu_weighted.py's: a row of length T and one of length 0; weights with a negative one and one exactly 0."""
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    w = rng.standard_normal(B).astype(np.float32)
    w[0], w[1], w[2], w[3] = -abs(w[0]) - 0.25, abs(w[1]) + 0.25, 0.0, abs(w[3]) + 0.25
    return lens, w


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
# (V, ld, one logit of +100): ld a multiple of 4 keeps V <= 16384 on the register ladder; ld = 97 makes the rows unaligned -> streaming
ROW_CASES = [(V, -(-V // 4) * 4, False) for V in (3, 97, 2048, 2049, 4097, 8193, 12289, 16383, 16384, 16385)] + \
            [(97, 97, False), (16384, 16384, True), (16385, 16388, True)]
M_ROWS, B_ROWS, SCALE = 6, 3, 1.0 / 7.0
W_ROWS = np.array([0.0, -1.5, 0.75], np.float32)   # caption 0 (rows 0, 3): weight 0; caption 1 (rows 1, 4): negative; row 4's target is -1


@functools.lru_cache(maxsize=None)
def row_case(V, hot):
    rng = np.random.default_rng(90000 + V + hot)
    z = (rng.standard_normal((M_ROWS, V)) * 3.0).astype(np.float32)
    crit = [c for c in xl.critical_columns(V)]
    tgt = np.array([crit[0], crit[0], crit[1 % len(crit)], 1 % V, -1, int(rng.integers(0, V))], np.int32)
    if hot:
        assert tgt[2] != V // 2
        z[2, V // 2] = 100.0        # a non-target column of an active row: its plain term is about -100
    clean = z.copy()
    for m in (0, 3, 4):             # the inactive rows: never read
        z[m] = np.nan
    return z, clean, tgt


@functools.lru_cache(maxsize=None)
def row_reference(V, hot, eps, weighted=True):
    z, clean, tgt = row_case(V, hot)
    if not weighted:   # every weight 1: rows 0 and 3 are active, so they hold numbers
        return smr.xent_rows(np.where(np.isnan(z) & (np.arange(M_ROWS)[:, None] != 4), clean, z), tgt, eps, scale=float(np.float32(SCALE)))
    return smr.xent_rows(z, tgt, eps, row_w=W_ROWS, B=B_ROWS, scale=float(np.float32(SCALE)))


def bf16_round(a):
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy().astype(np.float64)


@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("V,ld,hot", ROW_CASES)
def test_kernel_alone_on_every_rung(V, ld, hot, eps):
    """Measured on an MI355X, worst over all cases of this test (it prints every figure under -s): row terms 1.2e-7 relative,
    d(logits) 0.29 of its bound, |row sum| 6.7e-7 |row scale|.  No bound was widened."""
    ctx = L.Context(16, 16, 16, 17, max_B=4, max_T=1)
    for weighted in (True, False):
        _kernel_alone(ctx, V, ld, hot, eps, weighted)
    ctx.close()


def _kernel_alone(ctx, V, ld, hot, eps, weighted):
    z, clean, tgt = row_case(V, hot)
    if not weighted:
        z = np.where(np.isnan(z) & (np.arange(M_ROWS)[:, None] != 4), clean, z)
    epsf = float(np.float32(eps))
    terms, ll, dlog = row_reference(V, hot, epsf, weighted)
    buf = torch.zeros((M_ROWS, ld), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.as_tensor(z)
    logits = buf[:, :V]
    assert logits.stride(0) == ld and logits.data_ptr() % 16 == 0
    w_rows = W_ROWS[np.arange(M_ROWS) % B_ROWS].astype(np.float64) if weighted else np.ones(M_ROWS)
    s_row = np.abs(np.float64(np.float32(SCALE)) * w_rows)
    active = [m for m in range(M_ROWS) if tgt[m] >= 0 and w_rows[m] != 0]
    assert active == ([1, 2, 5] if weighted else [0, 1, 2, 3, 5])
    for out_dtype in (torch.float32, torch.bfloat16):
        d, t, l = L.xent_logits(ctx, logits, tgt, row_weights=W_ROWS if weighted else None, B=B_ROWS, scale=SCALE, label_smoothing=eps,
                                out_dtype=out_dtype, ld_d=ld if ld % 4 == 0 else None)
        d, t, l = d.to(torch.float32).cpu().numpy().astype(np.float64), t.cpu().numpy(), l.cpu().numpy()
        for m in range(M_ROWS):
            if m not in active:
                assert t[m] == 0.0 and l[m] == 0.0 and not d[m].any(), "inactive row %d" % m
                continue
            rel_t, rel_l = abs(t[m] - terms[m]) / abs(terms[m]), abs(l[m] - ll[m]) / abs(ll[m])
            bound = 1e-5 * np.abs(dlog[m]) + 2e-6 * s_row[m]
            if out_dtype == torch.float32:
                err = np.abs(d[m] - dlog[m])
                rowsum = abs(d[m].sum())
                print("V=%d ld=%d hot=%d eps=%g w=%d f32 row %d: term rel %.2e, ll rel %.2e, dlog worst err / bound %.3f, |row sum| / scale %.2e"
                      % (V, ld, hot, eps, weighted, m, rel_t, rel_l, (err / bound).max(), rowsum / s_row[m]))
                assert rowsum <= 1e-5 * s_row[m]
            else:
                want = bf16_round(dlog[m])
                ulp = np.where(dlog[m] != 0, 2.0 ** (np.floor(np.log2(np.abs(dlog[m]) + 1e-300)) - 7), 0.0)
                err = np.abs(d[m] - want)
                bound = bound + ulp
                print("V=%d ld=%d hot=%d eps=%g w=%d bf16 row %d: dlog worst err / bound %.3f" % (V, ld, hot, eps, weighted, m, (err / bound).max()))
            assert rel_t <= 1e-5 and rel_l <= 1e-5
            assert (err <= bound).all(), "row %d: %d elements outside the bound, worst %.3e" % (m, int((err > bound).sum()), (err / bound).max())


def test_xent_logits_without_smoothing_runs_the_masked_and_weighted_kernels():
    # smooth == 0: terms == ll_terms, and d(logits) is the one-hot form; a target >= V makes a row inactive instead of indexing past it
    ctx = L.Context(16, 16, 16, 17, max_B=4, max_T=1)
    V = 203
    z, clean, tgt = row_case(V, False)
    tgt = tgt.copy()
    tgt[3] = V + 5
    zz = clean.copy()
    zz[3] = zz[4] = np.nan
    for w in (None, W_ROWS):
        terms, ll, dlog = smr.xent_rows(zz, tgt, 0.0, row_w=w, B=B_ROWS, scale=float(np.float32(SCALE)))
        d, t, l = L.xent_logits(ctx, torch.as_tensor(zz).cuda(), tgt, row_weights=w, B=B_ROWS, scale=SCALE)
        d, t, l = d.cpu().numpy().astype(np.float64), t.cpu().numpy(), l.cpu().numpy()
        assert np.array_equal(t, l) and t[3] == 0.0 and t[4] == 0.0 and not d[3].any() and not d[4].any()
        np.testing.assert_allclose(t, ll, rtol=1e-5)
        np.testing.assert_allclose(d, dlog, rtol=1e-5, atol=2e-6 * SCALE * 1.5)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2. smooth == 0
def direct_loss_grad_smooth(ctx, param, f, tokens, lens, w, nt, pdrop, seed, smooth, sched=None, fed=None):
    """lrcn_loss_grad_smooth itself (L.lossgradient names it only for a positive label_smoothing) -> (grads, loss)."""
    tok = L._tokens(tokens, f.device)
    T, B = tok.shape
    la = L._lens(lens, T, B, nt)
    wa = L._row_weights(w, lens, B) if w is not None else None
    d, keep = L._dropout(pdrop, seed, None, None)
    ss = L._sched(sched, B) if sched is not None else None
    grads = [L.jl_empty(*t.shape) for t in param]
    out = C.c_double()
    ctx._call("lrcn_loss_grad_smooth", L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), la[1], wa[1] if wa else None, T, B, la[2],
              C.byref(d) if d else None, C.byref(ss) if ss is not None else None, C.c_void_p(fed.data_ptr()) if fed is not None else None,
              C.c_float(smooth), L._p9(grads), C.byref(out))
    return grads, out.value


@pytest.mark.parametrize("pdrop", [0.0, 0.4])
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_smooth_zero_is_bit_identical(dtype, n_layers, pdrop):
    B, T, E, H, V = 24, 6, 64, 64, 301
    rng, m, feats, tokens, ctx, param = make(11, B, T, E, H, V, dtype, n_layers, det=True)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    w = rng.standard_normal(B).astype(np.float32)
    w[2] = 0.0
    f = L.to_jl(feats)
    for kw, row_w in (({}, None), ({"row_weights": w}, w)):
        ga, la = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, **kw)
        ga = host(ga)
        assert any(np.abs(a).max() > 0 for a in ga)
        gb, lb = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, label_smoothing=0.0, **kw)
        assert la == lb
        same_bits(ga, host(gb), "label_smoothing=0.0")
        gc, lc = direct_loss_grad_smooth(ctx, param, f, tokens, lens, row_w, None, pdrop, 9, 0.0)
        assert la == lc and L.last_loss(ctx) == la
        same_bits(ga, host(gc), "lrcn_loss_grad_smooth(smooth = 0)")
        assert L.smooth_stats(ctx) == (la, la)
        assert L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, label_smoothing=0.0, **kw) == L.loss(ctx, param, f, tokens, pdrop=pdrop, seed=9,
                                                                                                                  lens=lens, **kw)
    # with a scheduled-sampling argument whose eps is 0 it is lrcn_loss_grad_sched's call
    gd, ld_ = L.lossgradient(ctx, param, f, tokens, pdrop=pdrop, seed=9, lens=lens, sched=(0.0, 1.0, 3))
    ge, le = direct_loss_grad_smooth(ctx, param, f, tokens, lens, None, None, pdrop, 9, 0.0, sched=(0.0, 1.0, 3))
    assert ld_ == le
    same_bits(host(gd), host(ge), "smooth = 0 with sched")
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the whole model, f32
@pytest.mark.parametrize("n_layers,masks,B,T,E,H,V", [(2, True, 13, 7, 52, 36, 97), (1, False, 11, 6, 40, 48, 203), (2, False, 6, 3, 16, 16, 16400)])
def test_whole_model_f32_vs_reference(n_layers, masks, B, T, E, H, V):
    rng, m, feats, tokens, ctx, param = make(B + T, B, T, E, H, V, F32, n_layers)
    lens, w = mixed_case(rng, B, T)
    assert (w < 0).any() and (w == 0).any() and (lens == 0).any() and (lens == T).any()
    kw = {}
    if masks:
        kw["mask1"] = ((rng.random((T + 1, B, E)) > 0.4) / 0.6).astype(np.float32)
        kw["mask2"] = ((rng.random((T + 1, B, H)) > 0.4) / 0.6).astype(np.float32)
    f = L.to_jl(feats)
    ib = orc.PARAM_NAMES.index("bout")
    for nt in (None, 3 * vr.norm_tokens_of(lens)):   # the batch's own count, and a "global" one
        ref, ref_nll, ref_g = smr.loss(m, feats, tokens, lens, EPS, norm_tokens=nt, row_w=w, want_grad=True, **kw)
        plain = sr.loss(m, feats, tokens, lens, sr.gold_inputs(tokens, lens), norm_tokens=nt, row_w=w, **kw)
        for _ in range(2):   # twice: scratch carries the first pass's values
            g, val = L.lossgradient(ctx, param, f, tokens, lens=lens, norm_tokens=nt, row_weights=w, label_smoothing=0.1, **kw)
            nll, smoothed = L.smooth_stats(ctx)
            print("f32 smooth: loss", val, "ref", ref, "rel", abs(val - ref) / abs(ref), "nll", nll, "ref", plain)
            assert abs(val - ref) <= 1e-5 * abs(ref)
            assert smoothed == val and abs(nll - plain) <= 1e-5 * abs(plain) and abs(ref_nll - plain) <= 1e-12 * abs(plain)
            grads_close_f32(g, ref_g)
            gb = L.from_jl(g[ib]).astype(np.float64)
            assert abs(gb.sum()) <= 1e-5 * np.abs(gb).sum() + 1e-7   # every d(logits) row sums to 0, so does their sum over the rows
        only = L.loss(ctx, param, f, tokens, lens=lens, norm_tokens=nt, row_weights=w, label_smoothing=0.1, **kw)
        assert abs(only - ref) <= 1e-5 * abs(ref)
    # equal lengths, no lens: lens[b] = T and the equal-length normaliser norm_B (T + 1)
    full = np.full(B, T, np.int32)
    ref, _, ref_g = smr.loss(m, feats, tokens, full, EPS, norm_tokens=(2 * B) * (T + 1), want_grad=True, **kw)
    g, val = L.lossgradient(ctx, param, f, tokens, norm_B=2 * B, label_smoothing=0.1, **kw)
    assert abs(val - ref) <= 1e-5 * abs(ref)
    grads_close_f32(g, ref_g, "equal lengths")
    ctx.close()


# ------------------------------------------------------------------------------------------------ 4. the whole model, bf16
@pytest.mark.parametrize("B", [256, 48])
def test_whole_model_bf16_vs_float64_reference(B):
    """256 rows: GEMM + cell kernel per recurrence step; 48 rows: the fused step kernels.  Against the float64 reference under
    parity_util.assert_bf16_near_f32_oracle's bounds (2e-2 on the loss and per tensor in norm): a missing eps onehot or eps / V term moves
    g_bout and g_Wout by about eps = 10 %.  No elementwise bf16 emulation exists for this form -- the emulating oracle does not implement
    label smoothing -- and the kernels' own bf16 rounding of d(logits) is held by test_kernel_alone_on_every_rung."""
    T, E, H, V = 5, 64, 64, 157
    rng, m, feats, tokens, ctx, param = make(B, B, T, E, H, V, BF16)
    lens, w = mixed_case(rng, B, T)
    ref, _, ref_g = smr.loss(m, feats, tokens, lens, EPS, row_w=w, want_grad=True)
    g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, row_weights=w, label_smoothing=0.1)
    print("bf16 smooth B=%d: loss" % B, val, "f64", ref)
    assert_bf16_near_f32_oracle(val, g, ref, ref_g, "smooth bf16 B=%d" % B)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. with scheduled sampling
def test_with_scheduled_sampling_the_draw_is_untouched():
    B, T, E, H, V = 8, 4, 32, 32, 61
    rng, m, feats, tokens, ctx, param = make(5, B, T, E, H, V, F32, det=True)
    lens = rng.integers(1, T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = T, 0
    w = rng.uniform(-1, 2, size=B).astype(np.float32)
    f = L.to_jl(feats)
    ss = (0.5, 1.0, 21, 500)
    _, _, fed0 = L.lossgradient(ctx, param, f, tokens, lens=lens, norm_tokens=40, row_weights=w, sched=ss, return_fed=True)
    fire = sr.coins(21, 0.5, lens, T, 500)
    assert fire.sum() > 0 and (fed0[fire] != sr.gold_inputs(tokens, lens)[fire]).any()
    g, val, fed = L.lossgradient(ctx, param, f, tokens, lens=lens, norm_tokens=40, row_weights=w, sched=ss, return_fed=True, label_smoothing=0.1)
    assert np.array_equal(fed, fed0)
    assert L.sched_stats(ctx) == (int(lens.sum()), int(fire.sum()))
    ref, _, ref_g = smr.loss(m, feats, tokens, lens, EPS, fed=fed, norm_tokens=40, row_w=w, want_grad=True)
    print("smooth under fed words: loss", val, "ref", ref, "drawn", int(fire.sum()))
    assert abs(val - ref) <= 1e-5 * abs(ref)
    grads_close_f32(g, ref_g)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. training step and trainer
@pytest.mark.parametrize("gclip", [0.0, ALWAYS])
def test_train_step_is_loss_grad_then_update(gclip):
    B, T, E, H, V = 16, 6, 64, 64, 211
    rng, m, feats, tokens, ctx, _ = make(31, B, T, E, H, V, BF16, det=True)
    lens, w = mixed_case(rng, B, T)
    f = L.to_jl(feats)
    res = []
    for fused in (True, False):
        param = L.model_from_arrays(m.p)
        optim = L.initparams(param)
        grads = [L.jl_empty(*t.shape) for t in param]
        losses = []
        for step in range(3):
            if fused:
                losses.append(L.train_step(ctx, param, optim, grads, f, tokens, pdrop=0.4, seed=step, want_loss=True, lens=lens, norm_tokens=200,
                                           row_weights=w, gclip=gclip, label_smoothing=0.1))
            else:
                _, val = L.lossgradient(ctx, param, f, tokens, pdrop=0.4, seed=step, grads=grads, lens=lens, norm_tokens=200, row_weights=w,
                                        label_smoothing=0.1)
                if gclip > 0:
                    L.grad_sumsq(ctx, grads)
                    L.clip_set(ctx, gclip)
                L.update(ctx, param, grads, optim, clipped=gclip > 0)
                losses.append(val)
        res.append((losses, host(param), host(optim.m), host(optim.v), optim.t))
    (la, pa, ma, va, ta), (lb, pb, mb, vb, tb) = res
    assert la == lb and ta == tb == 3
    same_bits(pa + ma + va, pb + mb + vb, "train_step")
    assert any(np.abs(a - L.from_jl(p0)).max() > 0 for a, p0 in zip(pa, L.model_from_arrays(m.p)) if a.size)
    # and it is not the unsmoothed step
    param = L.model_from_arrays(m.p)
    l0 = L.train_step(ctx, param, L.initparams(param), [L.jl_empty(*t.shape) for t in param], f, tokens, pdrop=0.4, seed=0, want_loss=True, lens=lens,
                      norm_tokens=200, row_weights=w, gclip=gclip)
    assert l0 != la[0]
    ctx.close()


@pytest.fixture
def one_rank_nccl():
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


def test_trainer_pipeline_and_sharded_update_give_the_single_calls_bits(monkeypatch, one_rank_nccl):
    """The single call is lrcn_train_step_smooth on a context with the update option the trainer's mode runs under: the group pipeline updates
    through LRCN_OPT_FUSED_UPDATE's Adam kernel (the trainer turns the option on), the sharded update through the plain one on its flat
    slice.  The two Adam kernels differ from each other in last bits (tests/test_gpu_fused_update.py compares them at atol 2e-5), so a
    single call under the other option equals the trainer's losses bit for bit -- a bf16 context rounds the difference away in its shadow
    weights -- and not its f32 parameters: that is what this test showed before it matched the option."""
    for k in ("LRCN_DP_FORCE_PIPELINE", "LRCN_DP_SPARSE_EMBED", "LRCN_DP_SHARD_ADAM", "LRCN_DP_GROUP_ADAM", "LRCN_DP_BUCKETS", "LRCN_DP_BACKEND",
              "LRCN_FUSED_UPDATE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LRCN_DP_FORCE_PIPELINE", "1")
    B, T, E, H, V = 16, 6, 64, 64, 211
    rng = np.random.default_rng(5)
    steps = []
    for _ in range(3):
        lens, w = mixed_case(rng, B, T)
        steps.append(((rng.standard_normal((B, 4096)) * 0.02).astype(np.float32), rng.integers(3, V, size=(T, B)).astype(np.int32), lens, w))

    def run(mode, fused=False):
        ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=BF16)
        try:
            ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
            param = L.initweights(ctx, seed=42)
            optim = L.initparams(param)
            losses = []
            if mode == "single":
                ctx.set_option(_lib.LRCN_OPT_FUSED_UPDATE, int(fused))
                grads = [L.jl_empty(*t.shape) for t in param]
                for k, (feats, toks, lens, w) in enumerate(steps):
                    losses.append(L.train_step(ctx, param, optim, grads, L.to_jl(feats), toks, pdrop=0.4, seed=(7 + k + 1) * 65536, want_loss=True,
                                               lens=lens, row_weights=w, label_smoothing=0.1))
                return host(param), losses
            tr = dp.DataParallelTrainer(ctx, param, optim, B, 1, 0, pdrop=0.4, seed=7, group=one_rank_nccl, backend="torch",
                                        shard_adam=(mode == "sharded"))
            assert tr.shard == (mode == "sharded") and (tr.shard or tr._group_pipeline()) and tr._fused == (mode == "pipeline")
            for feats, toks, lens, w in steps:
                tr.step(None, toks, feats=L.to_jl(feats), lens=lens, row_weights=w, label_smoothing=0.1)
                losses.append(tr.loss_value())
            torch.cuda.synchronize()
            out = (host(tr.param), losses)   # the trainer's own list: the exchange modes re-home the parameters into one flat buffer
            tr.close()
            return out
        finally:
            ctx.close()

    for mode in ("pipeline", "sharded"):
        pa, la = run("single", fused=(mode == "pipeline"))
        pb, lb = run(mode)
        print(mode, "losses", lb, "single", la, "max |d param|", max(float(np.abs(a - b).max()) for a, b in zip(pa, pb) if a.size))
        assert la == lb
        same_bits(pa, pb, mode)


def test_trainer_equal_length_step_and_the_abi_backend(monkeypatch):
    # without lens the trainer passes lens[b] = T and the global batch's normaliser, as it does for scheduled sampling
    for k in ("LRCN_DP_FORCE_PIPELINE", "LRCN_DP_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    B, T, E, H, V = 12, 5, 64, 64, 131
    rng, m, feats, tokens, ctx, _ = make(4, B, T, E, H, V, BF16, det=True)
    f = L.to_jl(feats)
    pa = L.model_from_arrays(m.p)
    tr = dp.DataParallelTrainer(ctx, pa, L.initparams(pa), B, 1, 0, pdrop=0.4, seed=7)
    tr.step(None, tokens, feats=f, label_smoothing=0.1)
    la = tr.loss_value()
    with pytest.raises(lrcn_amd.LrcnError):
        tr.step(None, tokens, feats=f, label_smoothing=1.5)
    torch.cuda.synchronize()
    pa = host(tr.param)
    tr.close()
    pb = L.model_from_arrays(m.p)
    lb = L.train_step(ctx, pb, L.initparams(pb), [L.jl_empty(*t.shape) for t in pb], f, tokens, pdrop=0.4, seed=8 * 65536, want_loss=True,
                      label_smoothing=0.1)
    assert la == lb
    same_bits(pa, host(pb), "equal-length trainer step")
    ctx.close()


def test_half_batches_with_the_whole_batchs_norm_tokens_sum_to_the_whole_gradient():
    B, T, E, H, V = 12, 5, 40, 48, 203
    rng, m, feats, tokens, ctx, param = make(17, B, T, E, H, V, F32)
    lens, w = mixed_case(rng, B, T)
    nt = vr.norm_tokens_of(lens)
    g, val = L.lossgradient(ctx, param, L.to_jl(feats), tokens, lens=lens, norm_tokens=nt, row_weights=w, label_smoothing=0.1)
    whole = host(g)
    parts, total = None, 0.0
    for rows in (slice(0, B // 2), slice(B // 2, B)):
        gh, vh = L.lossgradient(ctx, param, L.to_jl(np.ascontiguousarray(feats[rows])), np.ascontiguousarray(tokens[:, rows]), lens=lens[rows],
                                norm_tokens=nt, row_weights=w[rows], label_smoothing=0.1)
        gh = host(gh)
        parts = gh if parts is None else [a + b for a, b in zip(parts, gh)]
        total += vh
    assert abs(total - val) <= 1e-5 * abs(val)
    for n, a, b in zip(orc.PARAM_NAMES, parts, whole):
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-5, err_msg=n)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. argument checks
def test_the_five_exports_exist():
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
    import re
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.SMOOTH_HEADER).read(), flags=re.S)
    assert set(_lib.SMOOTH_SIGNATURES) == set(re.findall(r"\b(lrcn_[a-z0-9_]+)\s*\(", txt)) == set(NAMES)
    assert lib.lrcn_abi_version() == 5 == _lib.LRCN_ABI_VERSION


def test_a_bad_smooth_is_rejected_and_the_context_stays_usable():
    B, T, E, H, V = 6, 3, 16, 16, 23
    rng, m, feats, tokens, ctx, param = make(2, B, T, E, H, V, F32)
    lens = np.array([3, 0, 2, 1, 3, 2], np.int32)
    f = L.to_jl(feats)
    lib = _lib.lib()
    tok = L._tokens(tokens, f.device)
    la = L._lens(lens, T, B, None)
    grads = [L.jl_empty(*t.shape) for t in param]
    out = C.c_double()
    z = torch.zeros((4, 24), device="cuda")
    tg = torch.zeros(4, dtype=torch.int32, device="cuda")
    with pytest.raises(lrcn_amd.LrcnError):
        L.smooth_stats(ctx)   # no *_smooth call yet
    for bad in (float("nan"), -0.1, 1.5):
        assert lib.lrcn_loss_smooth(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), la[1], None, T, B, la[2], None, None, None, bad,
                                    C.byref(out)) == -1
        assert lib.lrcn_loss_grad_smooth(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), la[1], None, T, B, la[2], None, None, None, bad,
                                         L._p9(grads), C.byref(out)) == -1
        assert lib.lrcn_train_step_smooth(ctx._h, L._p9(param), L._p9(grads), L._p9(grads), L._p9(grads), L._ptr(f), C.c_void_p(tok.data_ptr()), la[1],
                                          None, T, B, la[2], None, None, bad, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, C.byref(out)) == -1
        assert lib.lrcn_xent_logits(ctx._h, C.c_void_p(z.data_ptr()), 24, C.c_void_p(tg.data_ptr()), None, 4, 4, 23, 1.0, bad, 0, None, 0, None,
                                    None) == -1
        with pytest.raises(lrcn_amd.LrcnError):
            L.loss(ctx, param, f, tokens, lens=lens, label_smoothing=bad)
    # what lrcn_loss_grad_sched rejects: a NULL lens, a length outside [0, T], a bad scheduled-sampling eps
    assert lib.lrcn_loss_smooth(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), None, None, T, B, la[2], None, None, None, 0.1,
                                C.byref(out)) == -1
    long_ = L._lens(np.array([T + 1] * B, np.int32), T, B, None)
    assert lib.lrcn_loss_smooth(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), long_[1], None, T, B, la[2], None, None, None, 0.1,
                                C.byref(out)) == -1
    ss = _lib.Sched(1.5, 1.0, 0, 0)
    assert lib.lrcn_loss_smooth(ctx._h, L._p9(param), L._ptr(f), C.c_void_p(tok.data_ptr()), la[1], None, T, B, la[2], None, C.byref(ss), None, 0.1,
                                C.byref(out)) == -1
    assert lib.lrcn_xent_logits(ctx._h, C.c_void_p(z.data_ptr()), 20, C.c_void_p(tg.data_ptr()), None, 4, 4, 23, 1.0, 0.1, 0, None, 0, None,
                                None) == -1   # ld < V
    ctx.sync()   # nothing was queued, nothing is pending
    ref, _ = smr.loss(m, feats, tokens, lens, EPS)
    val = L.loss(ctx, param, f, tokens, lens=lens, label_smoothing=0.1)
    assert abs(val - ref) <= 1e-5 * abs(ref)
    optim = L.initparams(param)
    with pytest.raises(lrcn_amd.LrcnError):
        L.train_step(ctx, param, optim, grads, f, tokens, lens=lens, label_smoothing=2.0)
    assert optim.t == 0
    ctx.close()
