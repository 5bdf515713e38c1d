"""GPU: the argument contract of the training entry points -- lrcn_loss*, lrcn_train_step* (plain, variable-length, clipped, weighted and
scheduled-sampling), lrcn_adam_update* (plain and clipped), lrcn_refresh_shadows_group, lrcn_grad_sumsq*, lrcn_clip_set -- on the raw C ABI: the return code of every bad call, the text it leaves in
lrcn_last_error (or that it leaves none), what a call that fails half-way has already done, and that max_norm = 0 is the unclipped step.

Every call is made with a known text in lrcn_last_error, so a bare return code is told from a failure with a message."""
import ctypes as C

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu

E = H = 8
V, B, T = 17, 2, 2
OK, EINVAL, ESTATE = 0, -1, -4
GROUPS, SLOTS = 5, 9          # LRCN_GRAD_GROUPS, LRCN_CLIP_SLOTS
MARK = "unknown option 999"   # what lrcn_set_option(ctx, 999, 0) leaves in lrcn_last_error

LOSS = "c p feats tokens T B norm_B drop loss"
LOSS_VAR = "c p feats tokens lens T B norm_tokens drop loss"
STEP = "c p g m v feats tokens T B norm_B drop step lr b1 b2 eps loss"
STEP_VAR = "c p g m v feats tokens lens T B norm_tokens drop step lr b1 b2 eps loss"
LOSS_W = LOSS_VAR.replace("lens", "lens row_w")
STEP_W = STEP_VAR.replace("lens", "lens row_w").replace("eps", "eps max_norm")
ADAM = "c p g m v step lr b1 b2 eps"
ADAM_GROUP = "c p g m v group step lr b1 b2 eps stream"
ADAM_FLAT = "c fw fg fm fv n step lr b1 b2 eps stream"
ARGS = {
    "lrcn_loss": LOSS, "lrcn_loss_grad": LOSS.replace("drop", "drop g"),
    "lrcn_loss_var": LOSS_VAR, "lrcn_loss_grad_var": LOSS_VAR.replace("drop", "drop g"),
    "lrcn_train_step": STEP, "lrcn_train_step_var": STEP_VAR,
    "lrcn_train_step_clip": STEP.replace("eps", "eps max_norm"), "lrcn_train_step_var_clip": STEP_VAR.replace("eps", "eps max_norm"),
    "lrcn_loss_w": LOSS_W, "lrcn_loss_grad_w": LOSS_W.replace("drop", "drop g"), "lrcn_train_step_w": STEP_W,
    "lrcn_loss_sched": LOSS_W.replace("drop", "drop ss fed logits"), "lrcn_loss_grad_sched": LOSS_W.replace("drop", "drop ss g fed logits"),
    "lrcn_train_step_sched": STEP_W.replace("drop", "drop ss"),
    "lrcn_adam_update": ADAM, "lrcn_adam_update_clipped": ADAM,
    "lrcn_adam_update_group": ADAM_GROUP, "lrcn_adam_update_group_clipped": ADAM_GROUP,
    "lrcn_adam_update_flat": ADAM_FLAT, "lrcn_adam_update_flat_clipped": ADAM_FLAT,
    "lrcn_refresh_shadows_group": "c p group stream", "lrcn_grad_group_wait": "c group stream",
    "lrcn_grad_sumsq": "c fg n slot stream", "lrcn_grad_sumsq_model": "c g group stream", "lrcn_clip_set": "c n_slots max_norm stream",
}
LOSSES = ("lrcn_loss", "lrcn_loss_grad", "lrcn_loss_var", "lrcn_loss_grad_var")
STEPS = ("lrcn_train_step", "lrcn_train_step_var", "lrcn_train_step_clip", "lrcn_train_step_var_clip")
VARS = ("lrcn_loss_var", "lrcn_loss_grad_var", "lrcn_train_step_var", "lrcn_train_step_var_clip")
WEIGHTED = ("lrcn_loss_w", "lrcn_loss_grad_w", "lrcn_train_step_w")               # lens and row_w required
SCHEDS = ("lrcn_loss_sched", "lrcn_loss_grad_sched", "lrcn_train_step_sched")   # lens and ss required, row_w optional
LATER_LOSSES, LATER_STEPS = WEIGHTED[:2] + SCHEDS[:2], (WEIGHTED[2], SCHEDS[2])
ADAMS = ("lrcn_adam_update", "lrcn_adam_update_clipped", "lrcn_adam_update_group", "lrcn_adam_update_group_clipped")
FLATS = ("lrcn_adam_update_flat", "lrcn_adam_update_flat_clipped")

_RAW = {}


def raw(name):
    """The library's function with the binding's signature, but a plain pointer where the binding wants a nine-pointer array: NULL can be
    passed for it.  (A CDLL of its own: the binding's argtypes stay as they are.)"""
    if not _RAW:
        _lib.lib()
        _RAW["lib"] = C.CDLL(_lib.LIB_PATH)
    if name not in _RAW:
        for table in (_lib.SIGNATURES, _lib.VARLEN_SIGNATURES, _lib.CLIP_SIGNATURES, _lib.WEIGHTED_SIGNATURES, _lib.SCHED_SIGNATURES):
            if name in table:
                res, args = table[name]
        fn = getattr(_RAW["lib"], name)
        fn.restype = res
        fn.argtypes = [C.c_void_p if a is _lib.P9 else a for a in args]
        _RAW[name] = fn
    return _RAW[name]


def i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def f32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def p9(ts, null=()):
    return _lib.P9(*[None if k in null else (t.data_ptr() or None) for k, t in enumerate(ts)])


class Rig:
    """One context, one model with its gradients and moments, one batch, and the default (valid) value of every argument."""

    def __init__(self, n_layers):
        self.ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_F32, n_layers=n_layers)
        self.ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
        self.model = L.initweights(self.ctx, seed=3)
        self.grads, self.m, self.v = (L.zeros_like_model(self.model) for _ in range(3))
        g = torch.Generator().manual_seed(5)
        self.feats = L.to_jl(torch.randn(B, _lib.CNNOUT, generator=g))
        self.tokens = torch.tensor([[3, 4], [5, 0]], dtype=torch.int32, device="cuda")
        self.lens = np.array([2, 1], np.int32)
        self.row_w = np.array([1.0, -0.5], np.float32)
        self.ss = _lib.Sched(0.5, 1.0, 7, 0)
        self.fed = torch.zeros((T + 1, B), dtype=torch.int32, device="cuda")
        self.logits = torch.zeros((T + 1, V, B), device="cuda")
        self.flat = [torch.zeros(16, device="cuda") for _ in range(4)]
        self.start = [t.clone() for t in self.model]
        torch.cuda.synchronize()
        self.defaults = dict(
            c=self.ctx._h, p=p9(self.model), g=p9(self.grads), m=p9(self.m), v=p9(self.v), feats=self.feats.data_ptr(),
            tokens=self.tokens.data_ptr(), lens=i32p(self.lens), row_w=f32p(self.row_w), ss=C.byref(self.ss),
            fed=self.fed.data_ptr(), logits=self.logits.data_ptr(), T=T, B=B, norm_B=B, norm_tokens=5, drop=None,
            step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_norm=1.0, loss=None, group=0, stream=None, n=16, slot=0, n_slots=SLOTS,
            fw=self.flat[0].data_ptr(), fg=self.flat[1].data_ptr(), fm=self.flat[2].data_ptr(), fv=self.flat[3].data_ptr())

    def reset(self):
        for dst, src in zip(self.model, self.start):
            dst.copy_(src)
        for t in self.m + self.v + self.grads:
            t.zero_()
        self.ctx.params_touched()

    def call(self, name, rc, text=None, **over):
        """Calls `name` with the defaults and `over`; asserts the return code and lrcn_last_error (text None: the call must leave none)."""
        h = self.ctx._h
        assert raw("lrcn_set_option")(h, 999, 0) == EINVAL
        vals = dict(self.defaults, **over)
        got = raw(name)(*[vals[a] for a in ARGS[name].split()])
        err = raw("lrcn_last_error")(h).decode()
        print("%s(%s) -> %d %r" % (name, ", ".join("%s=%r" % kv for kv in over.items()), got, err))
        assert got == rc
        assert err == (MARK if text is None else text)


@pytest.fixture(scope="module")
def two():
    rig = Rig(2)
    yield rig
    rig.ctx.close()


@pytest.fixture(scope="module")
def one():
    rig = Rig(1)
    yield rig
    rig.ctx.close()


def state_bits(rig):
    torch.cuda.synchronize()
    return [t.cpu().numpy().tobytes() for t in rig.model + rig.m + rig.v]


def test_a_valid_call_of_every_entry_point_succeeds(two):
    """The defaults are valid: what the other tests change is what is rejected."""
    for name in LOSSES + LATER_LOSSES + STEPS + LATER_STEPS + ADAMS + FLATS + ("lrcn_grad_group_wait", "lrcn_grad_sumsq", "lrcn_grad_sumsq_model",
                                                                               "lrcn_clip_set"):
        two.call(name, OK)
    two.ctx.sync()
    two.reset()


def test_null_handle_and_null_tensor_arrays(two):
    for name in LOSSES + LATER_LOSSES + STEPS + LATER_STEPS + ADAMS + FLATS + ("lrcn_refresh_shadows_group", "lrcn_grad_group_wait", "lrcn_grad_sumsq",
                                                                               "lrcn_grad_sumsq_model", "lrcn_clip_set"):
        vals = dict(two.defaults, c=None)
        assert raw(name)(*[vals[a] for a in ARGS[name].split()]) == EINVAL
    for name in LOSSES + LATER_LOSSES + STEPS + LATER_STEPS + ADAMS + ("lrcn_refresh_shadows_group",):
        for arg in "p g m v".split():
            if arg in ARGS[name].split():
                two.call(name, EINVAL, **{arg: None})
    two.call("lrcn_grad_sumsq_model", EINVAL, g=None)
    two.call("lrcn_grad_sumsq", EINVAL, fg=None)
    for name in LOSSES + LATER_LOSSES + STEPS + LATER_STEPS:
        two.call(name, EINVAL, feats=None)
        two.call(name, EINVAL, tokens=None)
    for name in FLATS:
        for arg in "fw fg fm fv".split():
            two.call(name, EINVAL, **{arg: None})


def test_step_below_one(two):
    for name in ADAMS + FLATS:
        two.call(name, EINVAL, step=0)
    # the unclipped steps find it in their update, after the pass has written the gradients; the clipped ones before anything runs
    for name, max_norm, ran in (("lrcn_train_step", 1.0, True), ("lrcn_train_step_var", 1.0, True), ("lrcn_train_step_clip", 0.0, True),
                                ("lrcn_train_step_var_clip", 0.0, True), ("lrcn_train_step_clip", 1.0, False),
                                ("lrcn_train_step_var_clip", 1.0, False), ("lrcn_train_step_w", 0.0, True), ("lrcn_train_step_sched", 0.0, True),
                                ("lrcn_train_step_w", 1.0, False), ("lrcn_train_step_sched", 1.0, False)):
        two.reset()
        before = state_bits(two)
        two.call(name, EINVAL, step=0, max_norm=max_norm)
        torch.cuda.synchronize()
        assert (float(two.grads[7].abs().sum()) > 0) == ran, name
        assert state_bits(two) == before, name
    two.reset()


def test_group_outside_its_range(two):
    for name in ("lrcn_adam_update_group", "lrcn_adam_update_group_clipped", "lrcn_refresh_shadows_group"):
        for group in (-1, GROUPS):
            two.call(name, EINVAL, "group=%d outside [0,%d)" % (group, GROUPS), group=group)
    for group in (-2, GROUPS):
        two.call("lrcn_grad_sumsq_model", EINVAL, "group=%d outside [-1,%d)" % (group, GROUPS), group=group)
    two.call("lrcn_grad_sumsq_model", OK, group=-1)
    for group in (-1, GROUPS):
        two.call("lrcn_grad_group_wait", EINVAL, group=group)
    two.call("lrcn_adam_update_group", EINVAL, group=-1, step=0)   # the step is looked at first


def test_refresh_shadows_group_needs_the_fused_update(two):
    two.call("lrcn_refresh_shadows_group", ESTATE, "lrcn_refresh_shadows_group needs LRCN_OPT_FUSED_UPDATE = 1 (the second shadow set)")
    two.ctx.set_option(_lib.LRCN_OPT_FUSED_UPDATE, 1)
    try:
        for group in range(GROUPS):
            two.call("lrcn_refresh_shadows_group", OK, group=group)
    finally:
        two.ctx.set_option(_lib.LRCN_OPT_FUSED_UPDATE, 0)
    two.ctx.sync()


def test_flat_update_lengths(two):
    for name in FLATS:
        two.call(name, OK, n=0, fw=None, fg=None, fm=None, fv=None)   # nothing to do: the pointers are not looked at
        two.call(name, EINVAL, n=-1)
        two.call(name, EINVAL, n=0, step=0)


def test_variable_length_arguments(two):
    bad_len = np.array([2, 3], np.int32)
    for name in VARS + WEIGHTED + SCHEDS:
        for max_norm in ((1.0, 0.0) if "max_norm" in ARGS[name].split() else (1.0,)):
            two.call(name, EINVAL, "lens is NULL", lens=None, max_norm=max_norm)
        two.call(name, EINVAL, "lens[1]=3 outside [0,%d]" % T, lens=i32p(bad_len))
        two.call(name, EINVAL, "norm_tokens=0 must be >= 1", norm_tokens=0)
        two.call(name, EINVAL, feats=None, lens=None)   # the NULL arrays are found before the NULL lens
    two.call("lrcn_train_step_var_clip", EINVAL, lens=None, step=0)   # clipped: the step before the lens
    two.call("lrcn_train_step_var", EINVAL, "lens is NULL", lens=None, step=0)
    for name in LATER_STEPS:   # as the clipped steps, by max_norm
        two.call(name, EINVAL, lens=None, step=0)
        two.call(name, EINVAL, "lens is NULL", lens=None, step=0, max_norm=0.0)


def test_row_weight_and_sched_arguments(two):
    """What the weighted and the scheduled-sampling entry points check on top: row_w, the lrcn_sched argument, and where in the order."""
    inf_w = np.array([1.0, np.inf], np.float32)
    for name in WEIGHTED:
        two.call(name, EINVAL, "row_w is NULL", row_w=None)
        two.call(name, EINVAL, "lens is NULL", lens=None, row_w=None)   # the NULL lens is found before the NULL row_w
        two.call(name, EINVAL, feats=None, lens=None, row_w=None)       # and the NULL arrays before both
    for name in SCHEDS:
        two.call(name, OK, row_w=None)                                  # optional here
        two.call(name, EINVAL, "the lrcn_sched argument is NULL", ss=None)
        two.call(name, EINVAL, "the lrcn_sched argument is NULL", ss=None, row_w=None)
        two.call(name, EINVAL, "lens is NULL", lens=None, ss=None)
        two.call(name, EINVAL, feats=None, lens=None, ss=None)
        for ss, text in ((_lib.Sched(1.5, 1.0, 7, 0), "sched eps=1.5 outside [0,1]"),
                         (_lib.Sched(0.5, -1.0, 7, 0), "sched temperature=-1 must be finite and >= 0"),
                         (_lib.Sched(0.5, float("inf"), 7, 0), "sched temperature=inf must be finite and >= 0"),
                         (_lib.Sched(0.5, 1.0, 7, -1), "sched row0=-1: rows [row0, row0 + B) must lie in [0, 2^32)"),
                         (_lib.Sched(0.5, 1.0, 7, 2 ** 32 - B + 1), "sched row0=%d: rows [row0, row0 + B) must lie in [0, 2^32)" % (2 ** 32 - B + 1))):
            two.call(name, EINVAL, text, ss=C.byref(ss))
        bad = _lib.Sched(1.5, 1.0, 7, 0)
        two.call(name, EINVAL, "T=%d outside [0,%d]" % (T + 1, T), ss=C.byref(bad), T=T + 1)   # the shapes before the sched values
        two.call(name, EINVAL, "sched eps=1.5 outside [0,1]", ss=C.byref(bad), norm_tokens=0)   # ... which come before the lengths
    for name in WEIGHTED + SCHEDS:
        two.call(name, EINVAL, "row_w[1]=inf is not finite", row_w=f32p(inf_w))
        two.call(name, EINVAL, "norm_tokens=0 must be >= 1", row_w=f32p(inf_w), norm_tokens=0)   # the lengths before the weights
    for name in LATER_STEPS:
        two.call(name, EINVAL, "max_norm is NaN", max_norm=float("nan"), step=0, lens=None)   # before the step and the lens
        two.call(name, EINVAL, max_norm=float("nan"), g=None)                                  # after the NULL arrays
    two.ctx.sync()
    two.reset()


def test_shapes_and_dropout_probability(two):
    d = _lib.Dropout(1.0, 7, None, None)
    for name in LOSSES + LATER_LOSSES + STEPS + LATER_STEPS:
        two.call(name, EINVAL, "pdrop=1 outside [0,1)", drop=C.byref(d))
        two.call(name, EINVAL, "T=%d outside [0,%d]" % (T + 1, T), T=T + 1)
        two.call(name, EINVAL, "B=%d outside [1,%d]" % (B + 1, B), B=B + 1)
    two.reset()


def test_max_norm_nan(two):
    for name in ("lrcn_train_step_clip", "lrcn_train_step_var_clip"):
        two.call(name, EINVAL, "max_norm is NaN", max_norm=float("nan"))
        two.call(name, EINVAL, "max_norm is NaN", max_norm=float("nan"), step=0)   # before the step
        two.call(name, EINVAL, max_norm=float("nan"), g=None)                      # after the NULL arrays
    two.call("lrcn_train_step_var_clip", EINVAL, "max_norm is NaN", max_norm=float("nan"), lens=None)
    two.call("lrcn_clip_set", EINVAL, "max_norm=0 is not > 0", max_norm=0.0)
    two.call("lrcn_clip_set", EINVAL, "max_norm=-1 is not > 0", max_norm=-1.0)


@pytest.mark.parametrize("plain, clip", [("lrcn_train_step", "lrcn_train_step_clip"), ("lrcn_train_step_var", "lrcn_train_step_var_clip")])
def test_max_norm_zero_is_the_unclipped_step(two, plain, clip):
    d = _lib.Dropout(0.25, 11, None, None)
    out = []
    for name in (plain, clip):
        two.reset()
        loss = C.c_double()
        for step in (1, 2):
            two.call(name, OK, max_norm=0.0, step=step, drop=C.byref(d), loss=C.byref(loss))
        out.append((state_bits(two), loss.value))
    assert out[0][0] != [t.cpu().numpy().tobytes() for t in two.start + two.m + two.v] and np.isfinite(out[0][1])
    assert out[0] == out[1]
    two.reset()


def test_slots_outside_their_range(two):
    for slot in (-1, SLOTS):
        two.call("lrcn_grad_sumsq", EINVAL, "slot=%d outside [0,%d)" % (slot, SLOTS), slot=slot)
    for n_slots in (0, SLOTS + 1):
        two.call("lrcn_clip_set", EINVAL, "n_slots=%d outside [1,%d]" % (n_slots, SLOTS), n_slots=n_slots)
    two.call("lrcn_clip_set", EINVAL, "n_slots=0 outside [1,%d]" % SLOTS, n_slots=0, max_norm=0.0)   # the slots before the norm
    two.call("lrcn_grad_sumsq", EINVAL, n=-1)


def test_a_null_tensor_in_slot_2(one, two):
    """W2, b2 and Wproj (slots 2, 3, 4) do not exist in the one-layer model: NULL is accepted there, and only there."""
    for rig, rc in ((one, OK), (two, EINVAL)):
        grads = p9(rig.grads, null=(2,))
        for name in ("lrcn_loss_grad", "lrcn_loss_grad_var", "lrcn_train_step", "lrcn_train_step_var_clip"):
            rig.call(name, rc, None if rc == OK else "null gradient tensor", g=grads)
        rig.call("lrcn_grad_sumsq_model", rc, g=grads, group=-1)
        rig.call("lrcn_loss", rc, None if rc == OK else "null parameter tensor", p=p9(rig.model, null=(2,)))
        rig.ctx.sync()
    assert one.model[2].numel() == 0 and two.model[2].numel() > 0
    two.reset()
