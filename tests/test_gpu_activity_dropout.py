"""GPU: dropout in activity training (include/lrcn_act_dropout.h): seeded masks against the host transcription of the generator bit for bit,
the input mask as a premultiplication, the identity forms, f32 parity with float64 autograd and bf16 parity with the rounding emulation of
tests/activity_drop_ref.py, the backward pass through the output mask, seeds, argument errors and the Python training path."""
import ctypes as C

import numpy as np
import pytest
import torch

import dropout_ref
from activity_drop_ref import emulated_drop, reference_drop, seeded_masks
from activity_ref import emulated
from lrcn_amd import _lib
from lrcn_amd import activity as A
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu
F32, BF16 = _lib.LRCN_F32, _lib.LRCN_BF16
SMALL = (72, 32, 7, 5, 3)       # a single ragged tile, M = 15
RAGGED = (136, 64, 11, 9, 15)   # F: three 64-tiles with a remainder of 8; M = 135: three row tiles with a remainder, ldM = 192 (padding)
PAPER = (4096, 256, 101, 16, 32)


def setup(F, H, C_, T, B, dtype=F32, det=False, seed=7, xs=1.0):
    """test_gpu_activity.py's setup(): random lens, first clip 1, last clip T."""
    m = A.ActivityModel(F, H, C_, max_B=B, max_T=T, dtype=dtype, deterministic=det, seed=seed)
    rng = np.random.default_rng(seed)
    x = (xs * rng.standard_normal((B * T, F))).astype(np.float32)
    lab = rng.integers(0, C_, B).astype(np.int32)
    lens = rng.integers(1, T + 1, B).astype(np.int32)
    lens[0], lens[-1] = 1, T
    return m, x, lab, lens


def host(m):
    return [L.from_jl(p).astype(np.float64) for p in m.params]


def call(m, x, lab, lens, T, **kw):
    """loss and clones of the four gradients, which are NaN before the call: a gradient that the call does not write fails every comparison"""
    for t in m.grads:
        t.fill_(float("nan"))
    loss = m.loss_grad(x, lab, lens, T, **kw)
    return loss, [t.clone() for t in m.grads]


def assert_same_bits(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for n, u, v in zip(A.PARAM_NAMES, a[1], b[1]):
        assert not torch.isnan(u).any(), (what, n)
        assert torch.equal(u, v), (what, n, float((u - v).abs().max()))


def host_grads(g):
    return [L.from_jl(t).astype(np.float64) for t in g]


# ---- 1. seeded equals explicit
SEEDED_CASES = [(0.5, 0.5, 12345), (0.9, 0.5, 12345), (0.4, 0.0, 12345), (0.0, 0.4, 12345),
                (dropout_ref.EDGE_P, 0.0, dropout_ref.EDGE_SEED)]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", [SMALL, RAGGED])
@pytest.mark.parametrize("case", SEEDED_CASES)
def test_seeded_equals_explicit_masks(case, shape, dtype):
    """(p_in, p_out, seed) against the same call with dropout_ref's arrays as explicit masks.  The last case holds, at the ragged shape, the
    element whose uniform equals p (T B F = 18360 > EDGE_INDEX; the small shape has 1080 elements and does not reach it): `>` keeps it out,
    `>=` would keep it in."""
    F, H, C_, T, B = shape
    p_in, p_out, seed = case
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=dtype, det=True)
    mi, mo = seeded_masks(seed, p_in, p_out, T, B, F, H)
    if seed == dropout_ref.EDGE_SEED and shape == RAGGED:
        assert T * B * F > dropout_ref.EDGE_INDEX
        assert dropout_ref.hash_uniform(seed, 1, [dropout_ref.EDGE_INDEX])[0] == np.float32(p_in)
        assert mi.reshape(-1)[dropout_ref.EDGE_INDEX] == 0
    a = call(m, x, lab, lens, T, pdrop_in=p_in, pdrop_out=p_out, drop_seed=seed)
    b = call(m, x, lab, lens, T, masks=(mi if p_in else None, mo if p_out else None))
    assert_same_bits(a, b, "seeded vs explicit")
    c = call(m, x, lab, lens, T, masks=(torch.as_tensor(mi).cuda(), torch.as_tensor(mo).cuda()))   # device tensors, ones on an identity side
    assert_same_bits(a, c, "seeded vs explicit device masks")
    l_fwd = m.loss_grad(x, lab, lens, T, grad=False, pdrop_in=p_in, pdrop_out=p_out, drop_seed=seed)   # grads == NULL: the loss only
    assert l_fwd == a[0]
    m.close()


# ---- 2. input dropout is a premultiplication
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_input_dropout_is_a_premultiplication(dtype):
    """p_out = 0: the call equals lrcn_act_loss_grad on feats * mask (float32 host product) bit for bit -- X, X' and their padding come out of
    act_frames_kernel<T, true> as out of act_frames_kernel<T, false>."""
    F, H, C_, T, B = RAGGED
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=dtype, det=True)
    seed, p_in = 99, 0.5
    mi = dropout_ref.drop_mult(seed, 1, p_in, T, B, F)
    xm = (x.reshape(B, T, F) * np.transpose(mi, (1, 0, 2))).astype(np.float32).reshape(B * T, F)
    plain = call(m, xm, lab, lens, T)
    assert_same_bits(call(m, x, lab, lens, T, pdrop_in=p_in, drop_seed=seed), plain, "seeded")
    assert_same_bits(call(m, x, lab, lens, T, masks=(mi, None)), plain, "explicit")
    assert plain[0] != call(m, x, lab, lens, T)[0]
    m.close()


# ---- 3. identity
def _raw(m, X, lab, lens, T, B, drop):
    i32 = lambda a: (C.c_int32 * len(a))(*[int(v) for v in a])  # noqa: E731
    for t in m.grads:
        t.fill_(float("nan"))
    d = C.c_double(-1.0)
    rc = _lib.lib().lrcn_act_loss_grad_drop(m._h, A.ActivityModel._p4(m.params), C.c_void_p(X.data_ptr()), i32(lab), i32(lens), T, B,
                                            C.byref(drop) if drop is not None else None, A.ActivityModel._p4(m.grads), C.byref(d))
    assert rc == 0
    return d.value, [t.clone() for t in m.grads]


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_identity_forms_give_the_plain_calls_bits(dtype):
    F, H, C_, T, B = RAGGED
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=dtype, det=True)
    X = L.to_jl(x)
    plain = call(m, X, lab, lens, T)
    assert_same_bits(_raw(m, X, lab, lens, T, B, None), plain, "drop = NULL")
    assert_same_bits(_raw(m, X, lab, lens, T, B, _lib.ActDropout(0.0, 0.0, 5, None, None)), plain, "p = 0, no masks")
    ones = (np.ones((T, B, F), np.float32), np.ones((T, B, H), np.float32))
    assert_same_bits(call(m, X, lab, lens, T, masks=ones), plain, "all-ones masks")
    assert_same_bits(call(m, X, lab, lens, T, masks=(None, ones[1])), plain, "all-ones output mask")
    m.close()


# ---- 4. f32 parity
def _f32_close(g, r, what):
    """test_gpu_activity.py's f32 bounds: rtol 1e-3, atol 1e-4 max|ref|"""
    for n, a, b in zip(A.PARAM_NAMES, g, r):
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-4 * np.abs(b).max(), err_msg="%s %s" % (what, n))


@pytest.mark.parametrize("shape", [SMALL, RAGGED])
def test_f32_parity_with_float64_autograd(shape):
    F, H, C_, T, B = shape
    m, x, lab, lens = setup(F, H, C_, T, B)
    seed = 4242
    mi, mo = seeded_masks(seed, 0.5, 0.5, T, B, F, H)
    loss, g = call(m, x, lab, lens, T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=seed)
    g = host_grads(g)
    rl, rg = reference_drop(*host(m), x, lab, lens, T, B, mi, mo)
    print("loss", loss, rl, "relative", abs(loss - rl) / abs(rl))
    assert abs(loss - rl) <= 1e-4 * abs(rl), (loss, rl)
    _f32_close(g, rg, "f32 %s" % (shape,))
    # a mask that is ignored fails here: every gradient is farther from the plain call's than the bound
    l0, g0 = call(m, x, lab, lens, T)
    assert abs(l0 - rl) > 1e-4 * abs(rl)
    for n, a, b in zip(A.PARAM_NAMES, host_grads(g0), rg):
        out = np.abs(a - b) > 1e-3 * np.abs(b) + 1e-4 * np.abs(b).max()
        print(n, "elements of the plain gradient outside the bound:", int(out.sum()), "of", out.size)
        assert out.any(), n
    m.close()


# ---- 5. bf16 parity
def _bf16_close(loss, g, el, eg):
    """_bf16_assert's bounds (test_gpu_activity.py): 5e-3 |e| + 2.5e-3 max|e| per element, the loss 1e-4 relative"""
    print("loss", loss, el, "relative", abs(loss - el) / abs(el))
    worst = []
    for n, a, e in zip(A.PARAM_NAMES, g, eg):
        d = np.abs(a - e)
        tol = 5e-3 * np.abs(e) + 2.5e-3 * np.abs(e).max()
        worst.append((n, int((d > tol).sum()), d.size, float((d / tol).max())))
        print("%s: %d of %d outside; worst %.3f of the bound (max|e| %.3e)" % (worst[-1] + (np.abs(e).max(),)))
    assert abs(loss - el) <= 1e-4 * abs(el), (loss, el)
    assert all(w[1] == 0 for w in worst), worst


@pytest.mark.parametrize("shape,p", [(RAGGED, (0.5, 0.5)), (PAPER, (0.9, 0.5))])
def test_bf16_parity_with_the_rounding_emulation(shape, p):
    """The paper's shape puts the fused recurrence (B = 32) between the two masks.  Features are scaled by sqrt(1 - p_in): the masked features
    keep the unit variance those bounds were set for."""
    F, H, C_, T, B = shape
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=BF16, xs=float(np.sqrt(1.0 - p[0])))
    seed = 31
    mi, mo = seeded_masks(seed, p[0], p[1], T, B, F, H)
    loss, g = call(m, x, lab, lens, T, pdrop_in=p[0], pdrop_out=p[1], drop_seed=seed)
    el, eg = emulated_drop(*host(m), x, lab, lens, T, B, mi, mo, bf16=True)
    _bf16_close(loss, host_grads(g), el, eg)
    # the masks are seen: the unmasked emulation is far outside the same bounds
    l0, g0, _, _ = emulated(*host(m), x, lab, lens, T, B, bf16=True)
    assert abs(loss - l0) > 1e-4 * abs(l0)
    m.close()


# ---- 6. backward through the output mask alone
def test_backward_through_the_output_mask_alone():
    F, H, C_, T, B = SMALL
    m, x, lab, lens = setup(F, H, C_, T, B)
    real = np.zeros((T, B), bool)
    for b in range(B):
        real[:lens[b], b] = True
    # the first seed at which at least one unit is dropped at every real step of every clip, and one is not (host search, nothing of the device)
    for seed in range(1000):
        mo = dropout_ref.drop_mult(seed, 2, 0.5, T, B, H)
        dead = ~(mo[real] != 0).any(0)          # [H]
        if dead.any() and not dead.all():
            break
    assert dead.any() and not dead.all()
    loss, g = call(m, x, lab, lens, T, pdrop_out=0.5, drop_seed=seed)
    g = host_grads(g)
    zero_rows = ~(g[2] != 0).any(1)
    np.testing.assert_array_equal(zero_rows, dead)
    rl, rg = reference_drop(*host(m), x, lab, lens, T, B, None, mo)
    assert abs(loss - rl) <= 1e-4 * abs(rl)
    _f32_close(g, rg, "output mask alone")   # dW and db among them: dh took the mask on its way into the recurrence
    m.close()


# ---- 7. seeds
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_seeds(dtype):
    F, H, C_, T, B = RAGGED
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=dtype, det=True)
    a = call(m, x, lab, lens, T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=1)
    b = call(m, x, lab, lens, T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=1)
    assert_same_bits(a, b, "same seed")
    c = call(m, x, lab, lens, T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=2)
    assert c[0] != a[0]
    big = call(m, x, lab, lens, T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=2 ** 63 + 1)   # the whole 64-bit key
    assert big[0] != a[0] and big[0] != c[0]
    m.close()


# ---- 8. argument errors
def test_argument_errors_before_gpu_work():
    F, H, C_, T, B = 16, 8, 3, 4, 2
    m, x, lab, lens = setup(F, H, C_, T, B)
    X = L.to_jl(x)
    for t in m.grads:
        t.fill_(123.0)
    torch.cuda.synchronize()
    Lb = _lib.lib()
    i32 = lambda a: (C.c_int32 * len(a))(*[int(v) for v in a])  # noqa: E731
    g4 = A.ActivityModel._p4(m.grads)
    p4 = A.ActivityModel._p4(m.params)
    D = _lib.ActDropout
    ok = D(0.5, 0.5, 1, None, None)
    ones = torch.ones(T * B * F, device="cuda")
    cases = [
        (i32(lab), i32(lens), T, B, D(1.0, 0.0, 1, None, None)),             # p_in = 1
        (i32(lab), i32(lens), T, B, D(0.0, -0.1, 1, None, None)),            # p_out < 0
        (i32(lab), i32(lens), T, B, D(float("nan"), 0.0, 1, None, None)),    # NaN
        (i32(lab), i32(lens), T, B, D(0.0, float("nan"), 1, None, None)),
        (i32(lab), i32(lens), T, B, D(1.5, 0.0, 1, ones.data_ptr(), None)),  # a mask does not excuse its p
        (i32(lab), i32(lens), T + 1, B, ok),                                 # check_call's: T > max_T
        (i32([0, C_]), i32(lens), T, B, ok),                                 # label >= C
        (i32(lab), i32([1, T + 1]), T, B, ok),                               # len > T
        (None, i32(lens), T, B, ok),                                         # no labels
    ]
    for lb, ln, t, b, d in cases:
        out = C.c_double(-1.0)
        assert Lb.lrcn_act_loss_grad_drop(m._h, p4, C.c_void_p(X.data_ptr()), lb, ln, t, b, C.byref(d), g4, C.byref(out)) == -1
        assert out.value == -1.0
        assert Lb.lrcn_act_last_error(m._h)
    torch.cuda.synchronize()
    for t in m.grads:
        assert bool((t == 123.0).all())
    with pytest.raises(A.LrcnError):
        m.loss_grad(x, lab, lens, T, pdrop_in=1.0)
    with pytest.raises(A.LrcnError):
        m.loss_grad(x, lab, lens, T, masks=(np.ones((T, B, F + 1), np.float32), None))
    m.close()


# ---- 9. the Python training path
def test_train_step_is_seeded_and_resumes(tmp_path):
    F, H, C_, T, B = SMALL
    rng = np.random.default_rng(0)
    batches = [((rng.standard_normal((B * T, F))).astype(np.float32), rng.integers(0, C_, B).astype(np.int32),
                np.array([1, 3, T], np.int32)) for _ in range(6)]
    models = [A.ActivityModel(F, H, C_, max_B=B, max_T=T, deterministic=True, seed=9) for _ in range(2)]
    assert models[0].drop_seed == 9
    losses = [[], []]
    for k in range(5):
        for i, m in enumerate(models):
            losses[i].append(m.train_step(*batches[k], T, lr=1e-2, pdrop_in=0.5, pdrop_out=0.5))
    assert losses[0] == losses[1]
    assert len(set(losses[0])) == 5
    for u, v in zip(models[0].params, models[1].params):
        assert torch.equal(u, v)
    # step k draws with drop_seed + k: the first step is loss_grad at seed 9 + 0
    fresh = A.ActivityModel(F, H, C_, max_B=B, max_T=T, deterministic=True, seed=9)
    assert fresh.loss_grad(*batches[0], T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=9) == losses[0][0]
    assert fresh.loss_grad(*batches[0], T, pdrop_in=0.5, pdrop_out=0.5, drop_seed=10) != losses[0][0]
    # save, load, one more step = the uninterrupted run
    ck = str(tmp_path / "act.npz")
    models[0].save(ck)
    assert int(np.load(ck)["drop_seed"]) == 9
    resumed = A.ActivityModel.load(ck, max_B=B, max_T=T)
    assert resumed.drop_seed == 9 and resumed.step == 5
    l_res = resumed.train_step(*batches[5], T, lr=1e-2, pdrop_in=0.5, pdrop_out=0.5)
    l_run = models[1].train_step(*batches[5], T, lr=1e-2, pdrop_in=0.5, pdrop_out=0.5)
    assert l_res == l_run
    for u, v in zip(resumed.params, models[1].params):
        assert torch.equal(u, v)
    # a checkpoint from before dropout (no drop_seed key) loads as before
    z = dict(np.load(ck))
    del z["drop_seed"]
    old = str(tmp_path / "old.npz")
    np.savez(old, **z)
    m_old = A.ActivityModel.load(old, max_B=B, max_T=T)
    assert m_old.drop_seed == 0 and m_old.step == 5
    for u, v in zip(m_old.params, models[0].params):
        assert torch.equal(u, v)
    for mm in models + [fresh, resumed, m_old]:
        mm.close()
