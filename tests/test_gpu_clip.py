"""GPU: clipping of the global gradient norm on the device (include/lrcn_clip.h) against its host restatement tests/clip_ref.py.

1. the sum of squares: within the worst-case rounding of ANY summation order of n non-negative doubles of the exactly rounded sum,
   |dev - fsum| <= (n + 2) 2^-53 fsum (squares of floats are exact in double; n - 1 additions, fsum's own rounding), and the same
   bits on every call, stream and pointer alignment;
2. lrcn_clip_set: clip_ref's scale to the bit, its norm to 1 ulp of double;
3. a clipped update is the plain update on clip_ref's pre-scaled gradient, bit for bit, on every route (whole model, groups, flat;
   fused with the shadow pass or not; f32 / bf16 shadows; one or two LSTM layers);
4. a non-finite gradient leaves w, m, v untouched -- and the fused update still writes the next step's shadow weights;
5. lrcn_train_step[_var]_clip equals [loss-gradient -> download -> clip_ref -> plain update] after every one of six steps;
6. the trainer (dp.py) clips on the device in every mode of its "torch" backend;
7. tools/lrcn.py --gclip prints its counters."""
import functools
import importlib
import json
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib, dp
from lrcn_amd import lrcn as L

import clip_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

E = H = 64
V, B, T = 300, 4, 5
ALWAYS = 1e-3   # far below any gradient norm met here: every step clips


def make_ctx(dtype=lrcn_amd.LRCN_BF16, n_layers=2, fused=False, det=True):
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=dtype, n_layers=n_layers)
    ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1 if det else 0)
    ctx.set_option(_lib.LRCN_OPT_FUSED_UPDATE, 1 if fused else 0)
    return ctx


def read_slots(ctx, n=9):
    ctx.sync()
    return L.clip_slots(ctx, n).cpu().numpy().copy()


def bits(arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def download(model):
    torch.cuda.synchronize()
    return [L.from_jl(t).copy() for t in model]


# ---------------------------------------------------------------------------------------------- 1. sum of squares
@functools.lru_cache(maxsize=None)
def wide_data(n):
    rng = np.random.default_rng(n + 1)
    a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 12, n)).astype(np.float32)
    return a, clip_ref.sumsq(a)


@pytest.fixture(scope="module")
def ctx0():
    ctx = make_ctx()
    yield ctx
    ctx.close()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 3, 255, 256, 257, 1023, 1000003])
def test_sumsq_is_within_the_summation_bound_and_reproducible(ctx0, n, off):
    a, want = wide_data(n)
    buf = torch.zeros(n + 8, device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    x = buf[off:off + n]
    x.copy_(torch.as_tensor(a))
    assert n == 0 or (x.data_ptr() % 16 == 0) == (off == 0)
    L.grad_sumsq(ctx0, x, slot=0)
    L.grad_sumsq(ctx0, x, slot=2)
    main = torch.cuda.current_stream()
    s2 = torch.cuda.Stream()
    s2.wait_stream(main)
    L.grad_sumsq(ctx0, x, slot=5, stream=s2)
    main.wait_stream(s2)
    s = read_slots(ctx0)
    print("n=%d off=%d dev=%r fsum=%r rel=%.3g bound=%.3g" % (n, off, s[0], want, abs(s[0] - want) / want if want else 0.0, (n + 2) * 2.0 ** -53))
    assert abs(s[0] - want) <= (n + 2) * 2.0 ** -53 * want
    assert s[0].tobytes() == s[2].tobytes() == s[5].tobytes()
    # ... and of the pointer's alignment: the other offset's value (same data) is the same double
    y = torch.zeros(n + 8, device="cuda", dtype=torch.float32)[1 - off:1 - off + n]
    y.copy_(torch.as_tensor(a))
    L.grad_sumsq(ctx0, y, slot=7)
    assert read_slots(ctx0)[7].tobytes() == s[0].tobytes()


def test_sumsq_of_values_whose_squares_overflow_float_is_finite(ctx0):
    n = 4099
    x = torch.full((n,), 1e30, device="cuda", dtype=torch.float32)
    L.grad_sumsq(ctx0, x, slot=1)
    got = read_slots(ctx0)[1]
    want = clip_ref.sumsq(np.full(n, 1e30, np.float32))
    assert math.isfinite(got) and abs(got - want) <= (n + 2) * 2.0 ** -53 * want


# ---------------------------------------------------------------------------------------------- 2. clip_set
@pytest.mark.parametrize("vals,max_norm", [((3.0, 4.0), 6.0), ((3.0, 4.0), 5.0), ((3.0, 4.0), 2.5),
                                           ((0.37, 1.9e-3, 12.25, 0.0, 7.0e2, 3.3, 1e-9, 41.0, 0.5), 5.0),
                                           ((0.37, 1.9e-3, 12.25, 0.0, 7.0e2, 3.3, 1e-9, 41.0, 0.5), 1e4)])
def test_clip_set_is_the_host_rule(vals, max_norm):
    ctx = make_ctx()
    try:
        x = torch.as_tensor(np.array(vals, np.float32)).cuda()
        for k in range(len(vals)):
            L.grad_sumsq(ctx, x[k:k + 1], slot=k)     # slot k = vals[k]^2, exactly
        slots = read_slots(ctx, len(vals))
        assert slots.tolist() == [float(np.float32(v)) ** 2 for v in vals]
        L.clip_set(ctx, max_norm, n_slots=len(vals))
        st = L.clip_stats(ctx)
        norm, scale, skip = clip_ref.clip_from_slots(slots.tolist(), max_norm)
        assert np.float32(st["last_scale"]).tobytes() == scale.tobytes(), (st, scale)
        assert abs(st["last_norm"] - norm) <= math.ulp(norm), (st, norm)
        assert st["last_skipped"] == 0 and st["steps"] == 1 and st["skipped"] == 0 and st["clipped"] == int(norm > max_norm)
        L.clip_set(ctx, max_norm, n_slots=len(vals))
        st = L.clip_stats(ctx)
        assert st["steps"] == 2 and st["clipped"] == 2 * int(norm > max_norm)
    finally:
        ctx.close()


def test_bad_arguments_are_rejected(ctx0):
    x = torch.zeros(4, device="cuda")
    for bad in (lambda: L.grad_sumsq(ctx0, x, slot=9), lambda: L.grad_sumsq(ctx0, x, slot=-1), lambda: L.clip_set(ctx0, float("nan")),
                lambda: L.clip_set(ctx0, 1.0, n_slots=10), lambda: L.clip_set(ctx0, 1.0, n_slots=0),
                lambda: L.grad_sumsq(ctx0, [x] * 9, group=5)):
        with pytest.raises(L.LrcnError):
            bad()


# ---------------------------------------------------------------------------------------------- 3. clipped Adam
def random_state(ctx, seed=11, gscale=0.1):
    """(parameters, gradient, m, v) as numpy arrays of the model's logical shapes."""
    rng = np.random.default_rng(seed)
    p = download(L.initweights(ctx, seed=42))
    g = [(rng.standard_normal(a.shape) * gscale).astype(np.float32) for a in p]
    m = [(rng.standard_normal(a.shape) * 0.01).astype(np.float32) for a in p]
    v = [(rng.standard_normal(a.shape) ** 2 * 1e-4).astype(np.float32) for a in p]
    return p, g, m, v


def device_state(p, g, m, v, t=3):
    param = L.model_from_arrays(p)
    optim = L.initparams(param)
    optim.m, optim.v, optim.t = L.model_from_arrays(m), L.model_from_arrays(v), t
    return param, L.model_from_arrays(g), optim


GROUP_ORDER = [3, 0, 4, 2, 1]


def do_update(ctx, form, param, grads, optim, clipped):
    if form == "whole":
        L.update(ctx, param, grads, optim, clipped=clipped)
    else:
        optim.t += 1
        for k in GROUP_ORDER:
            L.update_group(ctx, param, grads, optim, k, None, clipped=clipped)


def batch(seed=3):
    rng = np.random.default_rng(seed)
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.01).astype(np.float32))
    toks = torch.as_tensor(rng.integers(3, V, size=(T, B)).astype(np.int32)).cuda()
    return feats, toks


@pytest.mark.parametrize("form", ["whole", "groups"])
@pytest.mark.parametrize("n_layers", [2, 1])
@pytest.mark.parametrize("dtype", [lrcn_amd.LRCN_F32, lrcn_amd.LRCN_BF16])
@pytest.mark.parametrize("fused", [False, True])
def test_clipped_adam_is_plain_adam_on_prescaled_gradients(fused, dtype, n_layers, form):
    ctx = make_ctx(dtype, n_layers, fused)
    try:
        p, g, m, v = random_state(ctx)
        feats, toks = batch()
        for max_norm in (1.0, 1e30):
            pre, norm, scale, skip = clip_ref.clip(g, max_norm)
            assert not skip and (scale < 1.0) == (max_norm == 1.0)
            pa, ga, oa = device_state(p, g, m, v)
            L.grad_sumsq(ctx, ga)
            L.clip_set(ctx, max_norm)
            do_update(ctx, form, pa, ga, oa, True)
            loss_a = L.loss(ctx, pa, feats, toks)           # fused: reads the shadows the clipped kernel wrote
            ctx.params_touched()
            assert L.loss(ctx, pa, feats, toks) == loss_a   # ... which are those of the updated parameters
            assert bits(download(ga)) == bits(g)            # the gradient is not scaled in place
            st = L.clip_stats(ctx)
            assert np.float32(st["last_scale"]).tobytes() == scale.tobytes()
            # norm <= max_norm: the plain update on g itself (pre is g then)
            pb, gb, ob = device_state(p, pre, m, v)
            do_update(ctx, form, pb, gb, ob, False)
            loss_b = L.loss(ctx, pb, feats, toks)
            for name, a, b in (("p", pa, pb), ("m", oa.m, ob.m), ("v", oa.v, ob.v)):
                assert bits(download(a)) == bits(download(b)), (name, max_norm)
            assert loss_a == loss_b and oa.t == ob.t
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_clipped_flat_adam_is_plain_adam_on_prescaled_gradients(ctx0, n):
    rng = np.random.default_rng(n)
    w, g, m = ((rng.standard_normal(n) * s).astype(np.float32) for s in (1.0, 0.1, 0.01))
    v = (rng.standard_normal(n) ** 2 * 1e-4).astype(np.float32)
    max_norm = 0.05
    (pre,), norm, scale, skip = clip_ref.clip([g], max_norm)
    assert scale < 1.0

    class Opt:
        t, lr, beta1, beta2, eps = 4, 1e-3, 0.9, 0.999, 1e-8
    dev = lambda a: torch.as_tensor(a).cuda()
    wa, ga, ma, va = dev(w), dev(g), dev(m), dev(v)
    L.grad_sumsq(ctx0, ga, slot=0)
    L.clip_set(ctx0, max_norm, n_slots=1)
    L.update_flat(ctx0, wa, ga, ma, va, Opt, clipped=True)
    wb, gb, mb, vb = dev(w), dev(pre), dev(m), dev(v)
    L.update_flat(ctx0, wb, gb, mb, vb, Opt)
    torch.cuda.synchronize()
    for a, b in ((wa, wb), (ma, mb), (va, vb)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert ga.cpu().numpy().tobytes() == g.tobytes()
    assert not np.array_equal(wa.cpu().numpy(), w)


# ---------------------------------------------------------------------------------------------- 4. non-finite gradient
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("tensor,value", [(6, float("nan")), (8, float("inf"))])
def test_a_non_finite_gradient_skips_the_update(fused, tensor, value):
    """(The host path this replaces computed gclip / norm = NaN or 0 here and wrote it into every parameter and moment.)"""
    ctx = make_ctx(fused=fused)
    try:
        p, g, m, v = random_state(ctx)
        g[tensor].reshape(-1)[g[tensor].size // 3] = value
        feats, toks = batch()
        pa, ga, oa = device_state(p, g, m, v)
        loss0 = L.loss(ctx, pa, feats, toks)
        L.grad_sumsq(ctx, ga)
        L.clip_set(ctx, 5.0)
        L.update(ctx, pa, ga, oa, clipped=True)
        loss1 = L.loss(ctx, pa, feats, toks)   # fused: from the shadow set the skipped update wrote
        st = L.clip_stats(ctx)
        assert st["skipped"] == 1 and st["last_skipped"] == 1 and st["clipped"] == 0 and st["steps"] == 1 and st["last_scale"] == 1.0
        assert not math.isfinite(st["last_norm"])
        assert bits(download(pa)) == bits(p) and bits(download(oa.m)) == bits(m) and bits(download(oa.v)) == bits(v)
        assert loss1 == loss0 and math.isfinite(loss1)
        assert oa.t == 4   # the caller's step advances all the same
        # the next, finite step is an ordinary one
        g2 = random_state(ctx, seed=12)[1]
        pre, norm, scale, skip = clip_ref.clip(g2, 5.0)
        for t, src in zip(ga, L.model_from_arrays(g2)):
            t.copy_(src)
        L.grad_sumsq(ctx, ga)
        L.clip_set(ctx, 5.0)
        L.update(ctx, pa, ga, oa, clipped=True)
        loss2 = L.loss(ctx, pa, feats, toks)
        pb, gb, ob = device_state(p, pre, m, v, t=4)
        L.update(ctx, pb, gb, ob)
        assert bits(download(pa)) == bits(download(pb)) and loss2 == L.loss(ctx, pb, feats, toks)
        assert L.clip_stats(ctx)["skipped"] == 1
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 5. train_step_clip
STEPS = 6
LENS = [[5, 3, 0, 4], [2, 5, 5, 1], [4, 4, 3, 5], [1, 0, 2, 3], [5, 5, 4, 4], [3, 2, 5, 0]]


def step_inputs(k, seed0=100):
    return batch(seed0 + k)


def composed_run(var, max_norm, steps=STEPS, norm_B=None, seed_of=lambda k: 1000 + k, inputs=step_inputs, fused=False):
    """The reference, from entry points older than the feature: lrcn_loss_grad[_var] -> download -> clip_ref -> lrcn_adam_update on the
    pre-scaled gradient.  -> per step (parameter bits, loss, norm, clipped?)."""
    ctx = make_ctx(fused=fused)
    try:
        param = L.initweights(ctx, seed=42)
        optim = L.initparams(param)
        out = []
        for k in range(steps):
            feats, toks = inputs(k)
            grads, val = L.lossgradient(ctx, param, feats, toks, norm_B=norm_B, pdrop=0.4, seed=seed_of(k), lens=LENS[k] if var else None)
            g = download(grads)
            if max_norm is None:
                pre, norm, scale = g, clip_ref.clip_from_slots([clip_ref.sumsq(a) for a in g], 1.0)[0], np.float32(1)
            else:
                pre, norm, scale, skip = clip_ref.clip(g, max_norm)
                assert not skip
            L.update(ctx, param, L.model_from_arrays(pre), optim)
            out.append((bits(download(param)), val, norm, bool(scale < 1.0)))
        return out
    finally:
        ctx.close()


def device_run(var, max_norm, steps=STEPS):
    ctx = make_ctx()
    try:
        param = L.initweights(ctx, seed=42)
        optim = L.initparams(param)
        grads = L.zeros_like_model(param)
        out = []
        for k in range(steps):
            feats, toks = step_inputs(k)
            val = L.train_step(ctx, param, optim, grads, feats, toks, pdrop=0.4, seed=1000 + k, want_loss=True, lens=LENS[k] if var else None,
                               gclip=max_norm)
            out.append((bits(download(param)), val))
        return out, (L.clip_stats(ctx) if max_norm else None)
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def unclipped_reference(var):
    return composed_run(var, None)


@pytest.mark.parametrize("which", ["never", "always", "median"])
@pytest.mark.parametrize("var", [False, True])
def test_train_step_clip_follows_the_composed_reference(var, which):
    base = unclipped_reference(var)
    norms = [r[2] for r in base]
    max_norm = {"never": 1e30, "always": ALWAYS, "median": float(np.float32(np.median(norms)))}[which]
    ref = base if which == "never" else composed_run(var, max_norm)
    n_clip = sum(r[3] for r in ref)
    print("var=%s %s max_norm=%r norms=%r clipped=%r" % (var, which, max_norm, [r[2] for r in ref], [r[3] for r in ref]))
    if which == "never":
        assert n_clip == 0
    elif which == "always":
        assert n_clip == STEPS
    else:   # from the reference run alone
        assert n_clip >= 2 and STEPS - n_clip >= 2, [r[2] for r in ref]
    got, st = device_run(var, max_norm)
    for k in range(STEPS):
        assert got[k][1] == ref[k][1], ("loss", k)
        assert got[k][0] == ref[k][0], ("parameters", k)
    assert st["steps"] == STEPS and st["clipped"] == n_clip and st["skipped"] == 0
    if which == "never":   # ... and the plain entry point
        plain, _ = device_run(var, 0.0)
        assert [(b, l) for b, l in plain] == [(b, l) for b, l in got]


# ---------------------------------------------------------------------------------------------- 6. trainer modes
TR_STEPS, TR_SEED = 4, 7


def trainer_reference(max_norm):
    # the trainer's dropout seeds (rank 0), its normaliser, and LRCN_OPT_FUSED_UPDATE as the trainer sets it (the fused and the unfused
    # Adam kernels agree to a last bit, not bit for bit: tests/test_gpu_fused_update.py)
    return composed_run(False, max_norm, steps=TR_STEPS, norm_B=B, seed_of=lambda k: (TR_SEED + k + 1) * 65536, inputs=lambda k: batch(200 + k), fused=True)


@functools.lru_cache(maxsize=None)
def trainer_max_norms():
    norms = [r[2] for r in trainer_reference(None)]
    return ALWAYS, float(np.float32(np.median(norms)))


def trainer_run(gclip, shard=False, group=None):
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_BF16)
    try:
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
        param = L.initweights(ctx, seed=42)
        tr = dp.DataParallelTrainer(ctx, param, L.initparams(param), B, 1, 0, pdrop=0.4, seed=TR_SEED, group=group, backend="torch",
                                    shard_adam=shard, gclip=gclip)
        assert tr._dev_clip and tr.backend == "torch" and tr._fused == (not shard)
        out = []
        for k in range(TR_STEPS):
            feats, toks = batch(200 + k)
            tr.step(None, toks, feats=feats)
            out.append((download(param), tr.loss_value()))
        st = tr.clip_stats()
        flags = (tr.shard, tr._sparse_embed, tr._group_pipeline())
        tr.close()
        return out, st, flags
    finally:
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


@pytest.mark.parametrize("mode", ["plain", "pipeline", "sparse", "sharded"])
def test_trainer_clips_on_the_device_in_every_mode(monkeypatch, one_rank_nccl, mode):
    for k in ("LRCN_DP_FORCE_PIPELINE", "LRCN_DP_SPARSE_EMBED", "LRCN_DP_SHARD_ADAM", "LRCN_DP_GROUP_ADAM", "LRCN_DP_BUCKETS", "LRCN_DP_BACKEND",
              "LRCN_FUSED_UPDATE"):
        monkeypatch.delenv(k, raising=False)
    if mode in ("pipeline", "sparse"):
        monkeypatch.setenv("LRCN_DP_FORCE_PIPELINE", "1")
    monkeypatch.setenv("LRCN_DP_SPARSE_EMBED", "1" if mode == "sparse" else "0")
    for gclip in trainer_max_norms():
        ref = trainer_reference(gclip)
        n_clip = sum(r[3] for r in ref)
        got, st, (shard, sparse, pipe) = trainer_run(gclip, shard=(mode == "sharded"), group=one_rank_nccl if mode != "plain" else None)
        assert shard == (mode == "sharded") and sparse == (mode == "sparse") and pipe == (mode in ("pipeline", "sparse"))
        print("mode=%s gclip=%r norms=%r stats=%r" % (mode, gclip, [r[2] for r in ref], st))
        if mode == "sharded":
            # the same sum of squares partitioned by group slices instead of by tensor: the scale may differ in its last float bit
            np.testing.assert_allclose([l for _, l in got], [r[1] for r in ref], rtol=1e-6)
            want = [np.frombuffer(b, np.float32) for b in ref[-1][0]]
            for a, b in zip(got[-1][0], want):
                np.testing.assert_allclose(np.ascontiguousarray(a).ravel(), b, rtol=0, atol=1e-6)
        else:
            for k in range(TR_STEPS):
                assert got[k][1] == ref[k][1], ("loss", k)
                assert bits(got[k][0]) == ref[k][0], ("parameters", k)
            assert st["clipped"] == n_clip
        assert st["steps"] == TR_STEPS and st["skipped"] == 0
        if gclip == ALWAYS:
            assert st["clipped"] == TR_STEPS
        else:
            assert 0 < n_clip < TR_STEPS


@pytest.mark.parametrize("gclip", [ALWAYS, 1e30])
def test_activity_train_step_clips_like_the_composed_reference(gclip):
    from lrcn_amd import activity as A
    F, Hh, C_, Ta, Ba = 64, 32, 7, 5, 3
    rng = np.random.default_rng(7)
    x = rng.standard_normal((Ba * Ta, F)).astype(np.float32)
    lab = rng.integers(0, C_, Ba).astype(np.int32)
    lens = np.array([1, 3, Ta], np.int32)
    ma, mb = (A.ActivityModel(F, Hh, C_, max_B=Ba, max_T=Ta, dtype=_lib.LRCN_BF16, deterministic=True, seed=7) for _ in range(2))
    n_clip = 0
    for k in range(3):
        la = ma.train_step(x, lab, lens, Ta, lr=1e-2, gclip=gclip)
        lb = mb.loss_grad(x, lab, lens, Ta)
        pre, norm, scale, skip = clip_ref.clip(download(mb.grads), gclip)
        n_clip += int(scale < 1.0)
        for t, a in zip(mb.grads, pre):
            t.copy_(L.to_jl(a))
        mb.adam_step(1e-2)
        assert la == lb, k
        assert bits(download(ma.params)) == bits(download(mb.params)), k
    st = ma.clip_stats()
    assert st["steps"] == 3 and st["clipped"] == n_clip == (3 if gclip == ALWAYS else 0) and st["skipped"] == 0


# ---------------------------------------------------------------------------------------------- 7. CLI
def test_cli_gclip_prints_its_counters(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(40):
        n, v = nouns[img % 4], verbs[(img // 4) % 3]
        f = np.zeros(4096, np.float32)
        f[(img % 4) * 100:(img % 4) * 100 + 50] = 1.0
        f[1000 + ((img // 4) % 3) * 100:1000 + ((img // 4) % 3) * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns.append({"image_id": img, "caption": "A %s %s ." % (n, v)})
    from lrcn_amd import formats as fmt
    tr, va = str(tmp_path / "captions_train.json"), str(tmp_path / "captions_val.json")
    for p in (tr, va):
        with open(p, "w") as fh:
            json.dump({"annotations": anns}, fh)
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)
    argv = ["--coco", "--datafiles", tr, va, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "10", "--atype", "f32",
            "--seed", "3", "--train", "--epochs", "2", "--lr", "0.01", "--dropout", "0.0", "--gclip", "0.001"]
    assert cli.main(argv) == 0
    lines = capsys.readouterr().out.splitlines()
    epochs = [ln for ln in lines if ln.startswith("(:epoch")]
    clips = [ln for ln in lines if ln.startswith("(:gclip")]
    assert len(epochs) == 2 and len(clips) == 2
    # the (:epoch ...) line as test_gpu_cli.py parses it
    assert all(math.isfinite(float(ln.split(":loss,")[1].split(")")[0].split(",")[0])) for ln in epochs)
    assert lines.index(clips[0]) == lines.index(epochs[0]) + 1
    f = clips[-1].strip("()").split(", ")
    assert f[0] == ":gclip" and float(f[1]) == 0.001 and f[2] == ":clipped" and int(f[3]) > 0 and f[4] == ":skipped" and int(f[5]) == 0
    assert f[6] == ":last_norm" and float(f[7]) > 0.001
    assert int(clips[1].split(", ")[3]) > int(clips[0].split(", ")[3])
