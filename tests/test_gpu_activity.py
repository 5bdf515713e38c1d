"""GPU: activity recognition (include/lrcn_activity.h) against the float64 restatement of tests/activity_ref.py -- f32 and bf16 parity on
both recurrence routes, finite differences, structural identities, determinism, argument errors and learning an order-only task."""
import ctypes as C

import numpy as np
import pytest
import torch

from lrcn_amd import _lib
from lrcn_amd import activity as A
from lrcn_amd import lrcn as L

from activity_ref import emulated, order_task, reference

pytestmark = pytest.mark.gpu
F32, BF16 = _lib.LRCN_F32, _lib.LRCN_BF16


def setup(F, H, C_, T, B, dtype=F32, det=False, seed=7, xs=1.0):
    m = A.ActivityModel(F, H, C_, max_B=B, max_T=T, dtype=dtype, deterministic=det, seed=seed)
    rng = np.random.default_rng(seed)
    x = (xs * rng.standard_normal((B * T, F))).astype(np.float32)
    lab = rng.integers(0, C_, B).astype(np.int32)
    lens = rng.integers(1, T + 1, B).astype(np.int32)
    lens[0], lens[-1] = 1, T
    return m, x, lab, lens


def host(m):
    return [L.from_jl(p).astype(np.float64) for p in m.params]


def run(m, x, lab, lens, T):
    loss = m.loss_grad(x, lab, lens, T)
    g = [L.from_jl(t).astype(np.float64) for t in m.grads]
    cp, fp = m.predict(x, lens, T, frame_probs=True)
    return loss, g, L.from_jl(cp).astype(np.float64), L.from_jl(fp).astype(np.float64)


def assert_grads_close(g, r, rtol, what):
    for n, a, b in zip(A.PARAM_NAMES, g, r):
        np.testing.assert_allclose(a, b, rtol=rtol, atol=rtol * 0.1 * np.abs(b).max(), err_msg="%s %s" % (what, n))


@pytest.mark.parametrize("shape", [(64, 32, 7, 5, 3), (4096, 256, 101, 16, 32)])
def test_f32_parity(shape):
    F, H, C_, T, B = shape
    m, x, lab, lens = setup(F, H, C_, T, B)
    _f32_assert(m, x, lab, lens, T, B, "f32 %s" % (shape,))


def _f32_assert(m, x, lab, lens, T, B, what):
    loss, g, cp, fp = run(m, x, lab, lens, T)
    rl, rg, rc, rf = reference(*host(m), x, lab, lens, T, B)
    assert abs(loss - rl) <= 1e-4 * abs(rl), (loss, rl)
    assert_grads_close(g, rg, 1e-3, what)
    np.testing.assert_allclose(cp, rc, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(fp, rf, rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(cp.sum(0), 1.0, atol=1e-5)


def test_f32_finite_differences():
    F, H, C_, T, B = 64, 32, 7, 5, 3
    m, x, lab, lens = setup(F, H, C_, T, B)
    m.loss_grad(x, lab, lens, T)
    g = [L.from_jl(t).astype(np.float64) for t in m.grads]
    for k, p in enumerate(m.params):
        base = L.from_jl(p).copy()
        idx = np.argsort(-np.abs(g[k]).ravel())[:3]
        for i in idx:
            e = 1e-2 * max(1.0, abs(base.ravel()[i]))
            vals = []
            for s in (1, -1):
                q = base.copy()
                q.ravel()[i] += s * e
                p.copy_(torch.as_tensor(q))
                vals.append(m.loss_grad(x, lab, lens, T, grad=False))
            fd = (vals[0] - vals[1]) / (2 * e)
            assert abs(fd - g[k].ravel()[i]) <= 2e-2 * abs(g[k].ravel()[i]) + 1e-5, (A.PARAM_NAMES[k], i, fd, g[k].ravel()[i])
        p.copy_(torch.as_tensor(base))


def _bf16_check(shape, fused_env, monkeypatch):
    if fused_env is not None:
        monkeypatch.setenv("LRCN_LSTM_FUSED", fused_env)
    F, H, C_, T, B = shape
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=BF16)
    _bf16_assert(m, x, lab, lens, T, B)


def _bf16_assert(m, x, lab, lens, T, B):
    loss, g, cp, fp = run(m, x, lab, lens, T)
    P = host(m)
    el, eg, ec, ef = emulated(*P, x, lab, lens, T, B, bf16=True)
    rl, rg, _, _ = reference(*P, x, lab, lens, T, B)
    assert abs(loss - el) <= 1e-4 * abs(el), (loss, el)
    assert abs(loss - rl) <= 2e-2 * abs(rl), (loss, rl)
    for n, a, e, r in zip(A.PARAM_NAMES, g, eg, rg):
        d = np.abs(a - e)
        tol = 5e-3 * np.abs(e) + 2.5e-3 * np.abs(e).max()
        assert not (d > tol).any(), "%s: %d of %d outside; worst %.3e (max|ref| %.3e)" % (n, int((d > tol).sum()), d.size, d.max(), np.abs(e).max())
        assert np.linalg.norm(a - r) <= 2e-2 * np.linalg.norm(r), (n, np.linalg.norm(a - r) / np.linalg.norm(r))
    np.testing.assert_allclose(cp, ec, atol=2e-3)
    np.testing.assert_allclose(fp, ef, atol=2e-3)
    np.testing.assert_allclose(cp.sum(0), 1.0, atol=1e-5)


@pytest.mark.parametrize("shape", [(4096, 256, 101, 16, 128), (4096, 1024, 101, 16, 64)])
def test_bf16_parity_fused_steps(shape, monkeypatch):
    _bf16_check(shape, None, monkeypatch)


def test_bf16_parity_gemm_and_cell(monkeypatch):
    _bf16_check((4096, 1024, 101, 16, 64), "0", monkeypatch)


def test_bf16_parity_above_the_fused_batch(monkeypatch):
    _bf16_check((512, 256, 101, 8, 256), None, monkeypatch)


def test_first_step_is_lrcn_lstm():
    F, H, C_, T, B = 64, 32, 7, 5, 3
    m, x, lab, lens = setup(F, H, C_, T, B)
    _, fp = m.predict(x, None, T, frame_probs=True)
    fp = L.from_jl(fp)
    ctx = L.Context(F, H, 8, 8, max_B=B, max_T=1)
    x0 = np.stack([x[b * T] for b in range(B)])
    h, _ = L.lstm(ctx, m.params[0], m.params[1], L.jl_zeros(B, H), L.jl_zeros(B, H), L.to_jl(x0))
    z = L.from_jl(h).astype(np.float64) @ L.from_jl(m.params[2]) + L.from_jl(m.params[3])
    p = np.exp(z - z.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    for b in range(B):
        np.testing.assert_allclose(fp[:, b * T], p[b], rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_structure(dtype):
    F, H, C_, T, B = 128, 64, 11, 6, 5
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=dtype)
    # lens = NULL is lens = T
    full = np.full(B, T, np.int32)
    a = run(m, x, lab, None, T)
    b_ = run(m, x, lab, full, T)
    assert a[0] == b_[0]
    for u, v in zip(a[1] + [a[2], a[3]], b_[1] + [b_[2], b_[3]]):
        np.testing.assert_array_equal(u, v)
    # a mixed-length batch = each clip alone at T = len (probabilities), and the len-weighted combination (loss, gradients)
    loss, g, cp, _ = run(m, x, lab, lens, T)
    tot = float(lens.sum())
    acc_l, acc_g = 0.0, [np.zeros_like(t) for t in g]
    tol = 1e-5 if dtype == F32 else 5e-3
    for b in range(B):
        xb = x[b * T:b * T + lens[b]]
        lb, gb, cb, _ = run(m, xb, lab[b:b + 1], None, int(lens[b]))
        np.testing.assert_allclose(cp[:, b], cb[:, 0], rtol=tol, atol=tol * 1e-2)
        acc_l += lb * lens[b] / tot
        for k in range(4):
            acc_g[k] += gb[k] * lens[b] / tot
    assert abs(acc_l - loss) <= (1e-5 if dtype == F32 else 2e-3) * abs(loss)
    for k in range(4):
        err = np.linalg.norm(acc_g[k] - g[k]) / np.linalg.norm(g[k])
        assert err <= (1e-4 if dtype == F32 else 2e-2), (A.PARAM_NAMES[k], err)
    # permuting the clips permutes the outputs
    perm = np.random.default_rng(1).permutation(B)
    xp = np.concatenate([x[q * T:(q + 1) * T] for q in perm])
    lp, gp, cpp, fpp = run(m, xp, lab[perm], lens[perm], T)
    assert abs(lp - loss) <= 1e-6 * abs(loss)
    np.testing.assert_allclose(cpp, cp[:, perm], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(cp.sum(0), 1.0, atol=1e-5)


@pytest.mark.parametrize("dtype,B", [(F32, 32), (BF16, 128), (BF16, 512)])
def test_deterministic_repeats(dtype, B):
    F, H, C_, T = 4096, 256, 101, 16
    m, x, lab, lens = setup(F, H, C_, T, B, dtype=dtype, det=True)
    l1 = m.loss_grad(x, lab, lens, T)
    g1 = [t.clone() for t in m.grads]
    for t in m.grads:
        t.fill_(float("nan"))
    l2 = m.loss_grad(x, lab, lens, T)
    assert l1 == l2
    for n, u, v in zip(A.PARAM_NAMES, g1, m.grads):
        assert torch.equal(u, v), n
    c1 = m.predict(x, lens, T).clone()
    assert torch.equal(c1, m.predict(x, lens, T))


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
    cases = [
        (i32(lab), i32(lens), T + 1, B),          # T > max_T
        (i32(lab), i32(lens), 0, B),              # T < 1
        (i32(list(lab) * 2), None, T, B + 1),     # B > max_B
        (i32([0, C_]), i32(lens), T, B),          # label >= C
        (i32([-1, 0]), i32(lens), T, B),          # label < 0
        (i32(lab), i32([0, 2]), T, B),            # len < 1
        (i32(lab), i32([1, T + 1]), T, B),        # len > T
        (None, i32(lens), T, B),                  # no labels
    ]
    for lb, ln, t, b in cases:
        d = C.c_double(-1.0)
        assert Lb.lrcn_act_loss_grad(m._h, p4, C.c_void_p(X.data_ptr()), lb, ln, t, b, g4, C.byref(d)) == -1
        assert d.value == -1.0
    cp = L.jl_empty(C_, B + 1)
    assert Lb.lrcn_act_predict(m._h, p4, C.c_void_p(X.data_ptr()), i32([1, T + 1]), T, B, C.c_void_p(cp.data_ptr()), None) == -1
    assert Lb.lrcn_act_predict(m._h, p4, C.c_void_p(X.data_ptr()), None, T, B + 1, C.c_void_p(cp.data_ptr()), None) == -1
    assert Lb.lrcn_act_predict(m._h, p4, C.c_void_p(X.data_ptr()), None, T, B, None, None) == -1
    torch.cuda.synchronize()
    for t in m.grads:
        assert bool((t == 123.0).all())
    for cfg in ((0, 0, 8, 3, 4, 4, 0, 0), (0, 8, 0, 3, 4, 4, 0, 0), (0, 8, 8, 0, 4, 4, 0, 0)):
        h = C.c_void_p()
        assert Lb.lrcn_act_create(C.byref(_lib.ActConfig(*cfg)), C.byref(h)) == -1


def test_bf16_learns_the_order_of_two_patterns():
    F, H, C_, T, B = 16, 32, 2, 8, 64
    m = A.ActivityModel(F, H, C_, max_B=256, max_T=T, dtype=BF16, seed=5)
    xt, lt = order_task(256, T, F, seed=999)
    acc = 0.0
    for step in range(1, 801):
        x, lab = order_task(B, T, F, seed=step)
        m.train_step(x, lab, None, T, lr=1e-2)
        if step % 100 == 0:
            cp = L.from_jl(m.predict(xt, None, T))
            acc = float(np.mean(np.argmax(cp, 0) == lt))
            if acc >= 0.97:
                break
    assert acc >= 0.95, acc


def head_critical_classes(C_):
    """act_head_kernel<T, NQ> maps class c to thread c % 256 and register slot c // 256 (launch_head: NQ = 1, 2, 4, 8, 16 for C <= 256, 512,
    1024, 2048, 4096): the first and the last thread of the first two slots, both sides of the instantiation's last slot, the last class."""
    nq = next(q for q in (1, 2, 4, 8, 16) if C_ <= 256 * q)
    return nq, sorted({c for c in (0, 255, 256, 256 * (nq - 1) - 1, 256 * (nq - 1), C_ - 1) if 0 <= c < C_})


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C_", [256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096])
def test_head_instantiations(C_, dtype):
    """Every act_head_kernel<T, NQ> that launch_head can pick, at the last class count of each rung and the first of the next (the other
    tests stop at C = 101: NQ = 1 only).  The labels are critical classes and the output bias is N(0, 2^2) plus 4 on the critical classes,
    so each of them carries probability far above the tolerances and a slot that is dropped, doubled or scaled moves the loss, dbout, the
    clip and the frame probabilities.  References and bounds: test_f32_parity's against reference(), _bf16_check's against emulated().
    A local build (not kept) whose act_head_kernel<., 4> added the LAST slot's exponentials x 1.01 to the row sum failed C = 1024 in both
    types at the first assertion, the loss (8.9e-4 relative > 1e-4, against reference() and against emulated()), and no other case: at
    C = 513 the fourth slot (classes 768 ..) holds no class, the other counts are other instantiations."""
    F, H, T, B = 64, 32, 4, 3
    nq, crit = head_critical_classes(C_)
    m = A.ActivityModel(F, H, C_, max_B=B, max_T=T, dtype=dtype, seed=7)
    rng = np.random.default_rng(C_)
    x = rng.standard_normal((B * T, F)).astype(np.float32)
    lens = np.array([1, 4, 2], np.int32)
    lab = np.array([crit[-1], crit[-2], crit[len(crit) // 2]], np.int32)  # C - 1, the critical class below it, one of the middle
    bout = 2.0 * rng.standard_normal((1, C_))
    bout[0, crit] += 4.0
    m.params[3].copy_(torch.as_tensor(bout.astype(np.float32)))
    if dtype == F32:
        _f32_assert(m, x, lab, lens, T, B, "f32 head C=%d" % C_)
    else:
        _bf16_assert(m, x, lab, lens, T, B)
    m.close()


def test_more_than_4096_classes_are_refused():
    h = C.c_void_p()
    assert _lib.lib().lrcn_act_create(C.byref(_lib.ActConfig(0, 64, 32, 4097, 3, 4, 0, 0)), C.byref(h)) == -1
    assert not h.value and b"4096" in _lib.lib().lrcn_act_last_error(None)
