"""GPU: every route of the batched decode step (decode_route of csrc/decode.hip: tables, cell epilogue, plain) held value by value -- c1, c2,
h1, h2 and the logits after each of three steps -- to the float64 restatement of tests/decode_step_ref.py, by the bounds derived in that
module's docstring, through the test entry lrcn_debug_decode_steps (include/lrcn_decode_debug.h).  Arbitrary parent rows, tokens 0 and
V - 1, row counts with tails and across 256-row blocks; the route the library took is asserted before any value.

That these tests can fail: four local mutations of the library, each in bounds by construction, none kept; on the unmutated library all
cases pass with the worst error below 9 % of its bound (typically 0.3 .. 1 %) and 76 .. 98 % of the bf16 h held bit for bit.
  * `prow = row` in the LSTM_FWD epilogue of gemm_8p.hip (c_prev_idx ignored): the six tables and epi cases (tables-260, -515, -68,
    epi-by-width, epi-knob, epi-1f) fail at "step 1 c1", 98 .. 99 % of the entries outside a bound of 7e-7 by ~1e-3 .. 7e-3 (|c1| itself);
    the context-reuse test fails; the five plain cases pass, as they must (k_lstm_fwd reads no index), and so does the same-input test (step 0
    reads no parent).
  * decode_tables_build passing no bias to the dec_U2 GEMM: tables-260, -515, -68 fail at "step 0 c2", every entry outside a bound of
    5e-6 .. 2e-5 by ~0.2 .. 0.4; the same-input test fails on (epi-knob, tables-260, c2) and the context-reuse test fails; epi and plain pass.
  * k_row_div(st, c->dec_img, N * K, K + 1): the three tables cases fail at "step 0 c2" from the first row whose image changes (row 5 at
    per_image = 5, row 3 at 3), 93 .. 97 % of the entries outside a bound of 5e-6 .. 2e-5 by ~4e-4; same-input and context-reuse fail.
  * decode_prep_kernel copying E & ~7 embedding elements: epi-1f (E = 37) fails at "step 0 c1", 18428 of 18432 entries outside a bound of
    7e-7 by ~7e-4, and the context-reuse test (which runs epi-1f) fails; the two-layer epi cases have E = 40 and pass.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_step_ref as dr
import lrcn_amd
from lrcn_amd import _lib
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu

_RUNS = {}   # case -> (ref, device outputs, tokens, parents): one device run per case, shared by the tests below and left unchanged


def make_ctx(case, deterministic=False):
    bf16, layers, E, H1, H2, N, per_image, _, _ = dr.CASES[case]
    ctx = L.Context(E, H1, H2, dr.V, max_B=N * per_image, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16 if bf16 else lrcn_amd.LRCN_F32, n_layers=layers)
    if deterministic:
        ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    return ctx


def run_case(case, monkeypatch, ctx=None, parents=None):
    bf16, layers, E, H1, H2, N, per_image, knob, _ = dr.CASES[case]
    m, feats, tokens, par = dr.make_inputs(case)
    par = par if parents is None else parents
    for k in dr.KNOBS:
        monkeypatch.delenv(k, raising=False)
    if knob:
        monkeypatch.setenv(knob, "0")
    own = ctx is None
    if own:
        ctx = make_ctx(case)
    dev = L.debug_decode_steps(ctx, L.model_from_arrays(m.p), L.to_jl(feats), per_image, tokens, par)
    if own:
        ctx.close()
    return dr.Ref(m, feats, per_image, bf16), dev, tokens, par


def cached(case, monkeypatch):
    if case not in _RUNS:
        _RUNS[case] = run_case(case, monkeypatch)
    return _RUNS[case]


@pytest.mark.parametrize("case", list(dr.CASES))
def test_decode_step_route_and_values(case, monkeypatch):
    ref, dev, tokens, parents = cached(case, monkeypatch)
    assert dr.ROUTE_NAMES[dev["route"]] == dr.CASES[case][8], "decode_route took %s" % dr.ROUTE_NAMES[dev["route"]]
    figs = dr.check_case(ref, dev, tokens, parents)
    print(case, figs)


def test_same_inputs_give_the_same_first_step_on_all_three_routes(monkeypatch):
    """tables-260, epi-knob and plain-knob run identical inputs; after step 0 (no device state has entered yet) any two of them differ by at
    most the sum of their two bounds.  c1 hangs on the inputs alone.  c2 and the logits hang on each run's OWN h1 / h2 as well, which may be
    bf16 neighbours where h is loose: each run gets the reference fed its own h, and what the two references differ by is allowed on top
    (zero wherever the two runs stored the same h)."""
    runs = {c: cached(c, monkeypatch) for c in dr.SAME_INPUT}
    assert sorted(dr.ROUTE_NAMES[r[1]["route"]] for r in runs.values()) == ["epi", "plain", "tables"]
    ref, _, tokens, _ = runs[dr.SAME_INPUT[0]]
    for a in dr.SAME_INPUT:
        for b in dr.SAME_INPUT:
            if a >= b:
                continue
            da, db = runs[a][1], runs[b][1]
            # c1: both within dc1 of one reference.  c2 and the logits hang on each run's own h1 / h2, so each gets its own reference
            oa, ob = ref.step(tokens[0], None, da["h1"][0], da["h2"][0]), ref.step(tokens[0], None, db["h1"][0], db["h2"][0])
            assert np.all(np.abs(da["c1"][0].astype(np.float64) - db["c1"][0]) <= oa["dc1"] + ob["dc1"]), (a, b, "c1")
            for k, dk in (("c2", "dc2"), ("logits", "dlogits")):
                gap = np.abs(oa[k] - ob[k])    # what the two runs' own h1 / h2 (bf16 neighbours where loose) account for
                assert np.all(np.abs(da[k][0].astype(np.float64) - db[k][0]) <= oa[dk] + ob[dk] + gap), (a, b, k)


def test_a_used_context_gives_a_fresh_contexts_values(monkeypatch):
    """A second call on one context, after a call with other parents, against a fresh context: the swapped c pairs, dec_A1 / dec_A2 and their
    K padding start every call clean.  Under LRCN_OPT_DETERMINISTIC (no float-atomic split-K) the same kernels run on the same inputs in the
    same order, so the values are EQUAL; and the used context's values are held to the reference like any other run's."""
    for case in ("tables-260", "epi-knob", "plain-knob", "epi-1f"):
        N, per_image = dr.CASES[case][5:7]
        R = N * per_image
        _, _, tokens, parents = dr.make_inputs(case)
        other = parents.copy()
        other[1:] = (R - 1) - parents[1:]
        used, fresh = make_ctx(case, deterministic=True), make_ctx(case, deterministic=True)
        ref, first, _, _ = run_case(case, monkeypatch, ctx=used, parents=other)
        dr.check_case(ref, first, tokens, other)
        _, again, _, _ = run_case(case, monkeypatch, ctx=used)
        _, once, _, _ = run_case(case, monkeypatch, ctx=fresh)
        used.close()
        fresh.close()
        dr.check_case(ref, again, tokens, parents)
        assert again["route"] == once["route"] == dr.ROUTE_NAMES.index(dr.CASES[case][8])
        for k in ("h1", "c1", "h2", "c2", "logits"):
            if once[k] is not None:
                assert np.array_equal(again[k], once[k]), (case, k, float(np.abs(again[k] - once[k]).max()))


def test_every_refusal_leaves_the_outputs_untouched(monkeypatch):
    case = "plain-f32-1f"
    bf16, layers, E, H1, H2, N, per_image, _, _ = dr.CASES[case]
    two = dr.CASES["plain-f32"]
    m, feats, tokens, parents = dr.make_inputs(case)
    R = N * per_image
    for k in dr.KNOBS:
        monkeypatch.delenv(k, raising=False)
    ctx = L.Context(E, H1, H2, dr.V, max_B=R, max_T=1, n_layers=layers)
    ctx2 = L.Context(two[2], two[3], two[4], dr.V, max_B=8, max_T=1)
    m2 = dr.make_inputs("plain-f32")[0]
    param, param2 = L.model_from_arrays(m.p), L.model_from_arrays(m2.p)
    f = L.to_jl(feats)
    FILL = -7.5
    out = {k: torch.full((dr.STEPS, R, n), FILL, device="cuda") for k, n in (("h1", H1), ("c1", H1), ("h2", H2), ("c2", H2), ("logits", dr.V))}

    def struct(**kw):
        p9 = L._p9(param2 if kw.get("ctx") is ctx2 else param)
        a = dict(params=C.cast(p9, C.POINTER(C.c_void_p)), feats=f.data_ptr(), N=N, per_image=per_image, steps=dr.STEPS,
                 tokens=tokens.ctypes.data_as(C.POINTER(C.c_int32)), parents=parents.ctypes.data_as(C.POINTER(C.c_int32)),
                 h1=out["h1"].data_ptr(), h2=out["h2"].data_ptr(), c1=out["c1"].data_ptr(), c2=out["c2"].data_ptr(),
                 logits=out["logits"].data_ptr(), route=-9)
        a.update({k: v for k, v in kw.items() if k != "ctx"})
        d = _lib.DecodeDebug(**a)
        d._keep = p9
        return d

    def refused(what, cx=ctx, **kw):
        d = struct(ctx=cx, **kw)
        rc = _lib.lib().lrcn_debug_decode_steps(cx._h, C.byref(d))
        assert rc == -1 and _lib.lib().lrcn_last_error(cx._h), what   # LRCN_EINVAL, with a message
        assert d.route == -9, what
        torch.cuda.synchronize()
        for k, t in out.items():
            assert bool((t == FILL).all()), (what, k)

    assert _lib.lib().lrcn_debug_decode_steps(ctx._h, None) == -1
    for name in ("params", "feats", "tokens", "parents", "h1", "c1", "logits"):
        refused("NULL " + name, **{name: None})
    for name in ("h2", "c2"):   # required where the model has a second layer
        refused("NULL %s on LRCN-2f" % name, cx=ctx2, N=1, **{name: None})
    holes = L._p9(param)
    holes[6] = None
    refused("NULL parameter array", params=C.cast(holes, C.POINTER(C.c_void_p)))
    for name in ("N", "per_image", "steps"):
        refused(name + " = 0", **{name: 0})
        refused(name + " < 0", **{name: -1})
    refused("R > max_B", N=N + 1)
    refused("R > max_B by per_image", per_image=per_image + 1)
    for bad in (-1, dr.V):
        t = tokens.copy()
        t[dr.STEPS - 1, R - 1] = bad
        refused("token %d" % bad, tokens=t.ctypes.data_as(C.POINTER(C.c_int32)))
    for bad in (-1, R):
        p = parents.copy()
        p[1, R - 1] = bad
        refused("parent %d" % bad, parents=p.ctypes.data_as(C.POINTER(C.c_int32)))
    # and the same structure, unharmed, runs: LRCN-1f takes NULL h2 / c2
    d = struct(h2=None, c2=None)
    assert _lib.lib().lrcn_debug_decode_steps(ctx._h, C.byref(d)) == 0 and d.route == 0
    assert not bool((out["h1"] == FILL).any()) and bool((out["h2"] == FILL).all()) and bool((out["c2"] == FILL).all())
    ctx.close()
    ctx2.close()
