"""GPU: which entry point of the C ABI loss(), lossgradient() and train_step() reach, and with how many arguments, for every combination
of lens / row_weights / sched (and gclip); what they reject before any call is made; and the shape of lossgradient's sched extras.

The calls are recorded at Context._call, on a real context: every recorded call also runs."""
import itertools

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L
from lrcn_amd._lib import LrcnError

pytestmark = pytest.mark.gpu

E = H = 8
V, B, T = 17, 2, 2

# the first row whose argument is given applies: (loss, lossgradient, train_step with gclip > 0, train_step with gclip 0)
TABLE = (
    ("sched", ("lrcn_loss_sched", "lrcn_loss_grad_sched", "lrcn_train_step_sched", "lrcn_train_step_sched")),
    ("row_weights", ("lrcn_loss_w", "lrcn_loss_grad_w", "lrcn_train_step_w", "lrcn_train_step_w")),
    ("lens", ("lrcn_loss_var", "lrcn_loss_grad_var", "lrcn_train_step_var_clip", "lrcn_train_step_var")),
    (None, ("lrcn_loss", "lrcn_loss_grad", "lrcn_train_step_clip", "lrcn_train_step")),
)
COMBOS = list(itertools.product((False, True), (False, True), (None, 0.0, 0.5)))   # lens given, row_weights given, sched eps


def expected(kw, column):
    for key, names in TABLE:
        if key is None or kw.get(key) is not None:
            return names[column]


class Rig:
    def __init__(self):
        self.ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_F32)
        self.ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
        self.model = L.initweights(self.ctx, seed=3)
        self.grads = L.zeros_like_model(self.model)
        self.optim = L.initparams(self.model)
        g = torch.Generator().manual_seed(5)
        self.feats = L.to_jl(torch.randn(B, _lib.CNNOUT, generator=g))
        self.tokens = np.array([[3, 4], [5, 0]], np.int32)
        self.calls = []
        inner = self.ctx._call

        def recorder(name, *args):
            self.calls.append((name, args))
            return inner(name, *args)
        self.ctx._call = recorder

    def kwargs(self, lens, weights, eps):
        kw = {}
        if lens:
            kw["lens"] = np.array([2, 1], np.int32)
        if weights:
            kw["row_weights"] = np.array([1.0, -0.5], np.float32)
        if eps is not None:
            kw["sched"] = L.Sched(eps, 1.0, 7)
        return kw

    def one_call(self, fn, name):
        """Runs fn, which must make exactly one library call: `name`, with as many arguments as the binding declares after the handle."""
        del self.calls[:]
        out = fn()
        assert [c[0] for c in self.calls] == [name]
        assert len(self.calls[0][1]) == len(getattr(_lib.lib(), name).argtypes) - 1, name
        return out, self.calls[0][1]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    del r.ctx._call
    r.ctx.close()


@pytest.mark.parametrize("lens, weights, eps", COMBOS)
def test_symbol_and_argument_count(rig, lens, weights, eps):
    kw = rig.kwargs(lens, weights, eps)
    steps = [(1.0, 2), (0.0, 3), (None, 3)]   # gclip, the table's column
    if weights and not lens and eps is None:  # row_weights needs lens or sched: nothing is called, the step counter stays
        t0 = rig.optim.t
        del rig.calls[:]
        for fn in (lambda: L.loss(rig.ctx, rig.model, rig.feats, rig.tokens, **kw),
                   lambda: L.lossgradient(rig.ctx, rig.model, rig.feats, rig.tokens, grads=rig.grads, **kw),
                   lambda: L.train_step(rig.ctx, rig.model, rig.optim, rig.grads, rig.feats, rig.tokens, gclip=1.0, **kw),
                   lambda: L.train_step(rig.ctx, rig.model, rig.optim, rig.grads, rig.feats, rig.tokens, **kw)):
            with pytest.raises(LrcnError, match="row_weights needs lens"):
                fn()
        assert rig.calls == [] and rig.optim.t == t0
        return
    val, args = rig.one_call(lambda: L.loss(rig.ctx, rig.model, rig.feats, rig.tokens, **kw), expected(kw, 0))
    assert np.isfinite(val) and args[-1] is not None
    (g, val), args = rig.one_call(lambda: L.lossgradient(rig.ctx, rig.model, rig.feats, rig.tokens, grads=rig.grads, **kw), expected(kw, 1))
    assert g is rig.grads and np.isfinite(val)
    (g, val), args = rig.one_call(lambda: L.lossgradient(rig.ctx, rig.model, rig.feats, rig.tokens, grads=rig.grads, want_loss=False, **kw),
                                  expected(kw, 1))
    assert val is None and args[-1] is None   # want_loss=False passes NULL
    for gclip, column in steps:
        t0 = rig.optim.t
        more = {} if gclip is None else {"gclip": gclip}
        val, args = rig.one_call(lambda: L.train_step(rig.ctx, rig.model, rig.optim, rig.grads, rig.feats, rig.tokens, pdrop=0.25, seed=t0,
                                                      want_loss=True, **more, **kw), expected(kw, column))
        assert np.isfinite(val) and rig.optim.t == t0 + 1
        if expected(kw, column) in ("lrcn_train_step_w", "lrcn_train_step_sched"):
            assert args[-2] == float(gclip or 0.0)   # these two always receive gclip as their max_norm
        val, args = rig.one_call(lambda: L.train_step(rig.ctx, rig.model, rig.optim, rig.grads, rig.feats, rig.tokens, **more, **kw),
                                 expected(kw, column))
        assert val is None and args[-1] is None
    rig.ctx.sync()


def test_rejected_before_the_call(rig):
    t0 = rig.optim.t
    del rig.calls[:]
    lens = np.array([2, 1], np.int32)
    for extra in ({"return_fed": True}, {"return_logits": True}, {"return_fed": True, "lens": lens},
                  {"return_logits": True, "lens": lens, "row_weights": np.ones(B, np.float32)}):
        with pytest.raises(LrcnError, match="return_fed / return_logits need sched"):
            L.lossgradient(rig.ctx, rig.model, rig.feats, rig.tokens, grads=rig.grads, **extra)
    for bad in ({"row_weights": np.ones(B, np.float32)}, {"sched": (2.0, 1.0, 7)}, {"lens": np.array([2, 1, 1], np.int32)},
                {"lens": lens, "row_weights": np.ones(B + 1, np.float32)}):
        for gclip in (0.0, 1.0):
            with pytest.raises(LrcnError):
                L.train_step(rig.ctx, rig.model, rig.optim, rig.grads, rig.feats, rig.tokens, gclip=gclip, **bad)
    assert rig.calls == [] and rig.optim.t == t0


@pytest.mark.parametrize("eps", [0.0, 0.5])
def test_sched_extras_of_lossgradient(rig, eps):
    res, _ = rig.one_call(lambda: L.lossgradient(rig.ctx, rig.model, rig.feats, rig.tokens, grads=rig.grads, sched=L.Sched(eps, 1.0, 7),
                                                 return_fed=True, return_logits=True), "lrcn_loss_grad_sched")
    assert len(res) == 4
    g, val, fed, logits = res
    assert g is rig.grads and np.isfinite(val)
    assert fed.shape == (T + 1, B) and fed.dtype == np.int32
    assert logits.shape == (T + 1, B, V) and logits.dtype == np.float32 and np.isfinite(logits).all()
    assert (fed[0] == _lib.BOS).all()
    for extra, n in (({"return_fed": True}, 3), ({"return_logits": True}, 3), ({}, 2)):
        res, _ = rig.one_call(lambda: L.lossgradient(rig.ctx, rig.model, rig.feats, rig.tokens, grads=rig.grads, sched=(eps, 1.0, 7), **extra),
                              "lrcn_loss_grad_sched")
        assert len(res) == n
