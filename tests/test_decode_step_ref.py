"""CPU: the reference and the case table of tests/decode_step_ref.py, which tests/test_gpu_decode_step.py holds the device to.  No GPU.

1. The exact mode reproduces the oracle's lrcn_step (LRCN-2f and -1f) at float32 accuracy over two steps with identity parents; the
   bf16-emulating mode reproduces the same calls under orc.emulate_bf16().
2. Every case of the table predicts the route it names by a restatement of decode_route's rule, the table reaches every rule from both
   sides, and its inputs carry what they are there for (tokens 0, V - 1 and a repeat; parents with fixed points, repeats, rows outside the
   row's image and pairs across the 256-row boundary in both directions).
3. The cap: in every bf16 case less than a third of the h entries get the either-neighbour allowance -- computed from the reference
   alone, on a CPU stand-in for the device -- and that stand-in passes the GPU test's own assertions while a stand-in with one of the
   faults the GPU test is there for does not.
"""
import numpy as np
import pytest

import decode_step_ref as dr
from oracle import oracle as orc


# ---------------------------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("bf16", [False, True], ids=["exact", "bf16"])
@pytest.mark.parametrize("layers", [2, 1])
def test_reference_reproduces_the_oracles_step(layers, bf16):
    E, H1, H2, B = (5, 8, 12, 4) if layers == 2 else (5, 8, 8, 4)
    rng = np.random.default_rng(3)
    m = orc.init_weights(E, H1, H2, 19, seed=2, n_layers=layers)
    if layers == 2:
        m.p["b2"][:] = (rng.standard_normal(m.p["b2"].shape) * 0.5).astype(np.float32)
    m.p["bout"][:] = (rng.standard_normal(m.p["bout"].shape) * 0.5).astype(np.float32)
    feats = (rng.standard_normal((B, orc.CNNOUT)) * 0.05).astype(np.float32)
    tokens = rng.integers(0, 19, size=(2, B)).astype(np.int32)
    parents = np.tile(np.arange(B, dtype=np.int32), (2, 1))
    ref = dr.Ref(m, feats, 1, bf16)
    dev = dr.simulate(ref, tokens, parents)
    state = [np.zeros((B, H), np.float32, order="F") for H in ((H1, H1, H2, H2) if layers == 2 else (H1, H1))]
    x_cnn = orc.fa((orc.bf16_round(feats) if bf16 else feats).astype(np.float64) @ (orc.bf16_round(m.p["Wcnn"]) if bf16 else m.p["Wcnn"]).astype(np.float64))
    with orc.emulate_bf16(bf16):
        for s in range(2):
            logits = orc.lrcn_step(m, state, x_cnn, orc.fa(m.p["Wembed"][tokens[s]]))
            names = ("h1", "c1", "h2", "c2") if layers == 2 else ("h1", "c1")
            for k, st in zip(names, state):
                got = orc.bf16_round(st) if bf16 and k[0] == "h" else st     # the device stores h as bfloat16; the oracle rounds it on load
                np.testing.assert_allclose(got, dev[k][s], rtol=2e-6, atol=2e-7, err_msg="%s step %d" % (k, s))
            np.testing.assert_allclose(logits, dev["logits"][s], rtol=2e-6, atol=1e-6, err_msg="logits step %d" % s)


def test_bf16_round64_is_round_to_nearest_even_in_one_step():
    x = np.float32([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-5, 0.0, 0.33333334, 257.0])   # ties: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6
    assert np.array_equal(dr.bf16_round64(x), orc.bf16_round(x).astype(np.float64))
    assert dr.bf16_round64(1.00390625 + 1e-12) == 1.0078125    # float32 would round this to the tie first, and the tie down


# ---------------------------------------------------------------------------------------------- 2. the table
@pytest.mark.parametrize("case", list(dr.CASES))
def test_case_predicts_its_route_and_carries_its_edges(case):
    bf16, layers, E, H1, H2, N, per_image, knob, route = dr.CASES[case]
    R = N * per_image
    assert dr.predict_route(case) == route
    assert H2 % 2 == 0 and (layers == 2 or H1 == H2) and knob in (None,) + dr.KNOBS     # what lrcn_create accepts
    m, feats, tokens, parents = dr.make_inputs(case)
    assert tokens.shape == parents.shape == (dr.STEPS, R) and dr.STEPS == 3
    assert np.count_nonzero(feats[:, 0]) == N == np.count_nonzero(feats[:, -1]) and np.all(np.count_nonzero(feats, axis=1) == dr.FEAT_NNZ)
    assert float(np.abs(m.p["bout"]).min()) > 0 and (layers == 1 or float(np.abs(m.p["b2"]).mean()) > 0.3)
    for s in range(dr.STEPS):
        assert tokens[s].min() == 0 and tokens[s].max() == dr.V - 1 and len(set(tokens[s])) < R
    for s in range(1, dr.STEPS):
        p = parents[s]
        assert p.min() >= 0 and p.max() < R
        assert np.any(p == np.arange(R)) and len(set(p)) < R                              # fixed points, repeats
        assert np.any(p // per_image != np.arange(R) // per_image)                        # not confined to the row's image
        assert np.any(p != np.arange(R))
    assert dr.crosses_blocks(parents, R) == (R > 256)


def test_table_reaches_every_rule_from_both_sides():
    c = dr.CASES
    routes = {k: v[8] for k, v in c.items()}
    assert set(routes.values()) == set(dr.ROUTE_NAMES)
    rows = {k: v[5] * v[6] for k, v in c.items()}
    assert rows["plain-255"] == 255 and rows["epi-1f"] == 256 and rows["tables-260"] == 260 and rows["tables-515"] == 515   # the 256 rule; 2 and 3 row blocks
    assert c["epi-by-width"][3:5] == (64, 64) and c["tables-68"][3:5] == (68, 68)        # H > 64, from both sides
    assert c["plain-h70"][3] % 4 == 2 and c["tables-68"][3] % 8 == 4 and c["epi-1f"][2] % 8 == 5
    assert {c[k][7] for k in ("epi-knob", "plain-knob")} == set(dr.KNOBS)
    assert all(c[k][:7] == c["tables-260"][:7] for k in dr.SAME_INPUT)                   # identical shapes -> identical inputs
    a, b = dr.make_inputs("tables-260"), dr.make_inputs("plain-knob")
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(x, y) for x, y in zip(a[0].arrays(), b[0].arrays()))
    assert not c["plain-f32"][0] and not c["plain-f32-1f"][0] and c["plain-f32-1f"][1] == c["epi-1f"][1] == 1


# ---------------------------------------------------------------------------------------------- 3. the cap, and that the check can fail
_SIM = {}


def sim(case):
    if case not in _SIM:
        bf16, _, _, _, _, _, per_image, _, _ = dr.CASES[case]
        m, feats, tokens, parents = dr.make_inputs(case)
        ref = dr.Ref(m, feats, per_image, bf16)
        _SIM[case] = (ref, dr.simulate(ref, tokens, parents), tokens, parents)
    return _SIM[case]


@pytest.mark.parametrize("case", list(dr.CASES))
def test_loose_share_stays_under_the_cap_and_the_stand_in_passes(case):
    ref, dev, tokens, parents = sim(case)
    figs = dr.check_case(ref, dev, tokens, parents)
    print(case, [round(f["loose"], 3) for f in figs])
    if ref.bf16:
        assert all(f["loose"] < dr.MAX_LOOSE_SHARE for f in figs)
    else:
        assert all(f["h1_firm"] == 0.0 for f in figs)                     # f32: h is held by |h_dev - h| <= dh everywhere


def _with(a, s, v):
    a = a.copy()
    a[s] = v
    return a


def _step(ref, dev, tokens, parents, s):
    return ref.step(tokens[s], dr.gather(dev, s, parents), dev["h1"][s], dev["h2"][s] if ref.two else None)


@pytest.mark.parametrize("case", ["tables-260", "epi-1f", "plain-f32"])
def test_the_check_fails_for_a_stand_in_with_a_fault(case):
    ref, dev, tokens, parents = sim(case)
    R = parents.shape[1]
    ident = np.tile(np.arange(R, dtype=np.int32), (dr.STEPS, 1))
    # a dropped parent index: step 1's c1 computed from the row's own state
    bad = {**dev, "c1": _with(dev["c1"], 1, _step(ref, dev, tokens, ident, 1)["c1"].astype(np.float32))}
    with pytest.raises(AssertionError, match="step 1 c1"):
        dr.check_case(ref, bad, tokens, parents)
    # the logits' bias lost
    bad = {**dev, "logits": _with(dev["logits"], 0, dev["logits"][0] - ref.bout)}
    with pytest.raises(AssertionError, match="step 0 logits"):
        dr.check_case(ref, bad, tokens, parents)
    # one h entry one bf16 ulp (f32: 2^-9 relative) off where it is firm
    k = "h2" if ref.two else "h1"
    out = _step(ref, dev, tokens, parents, 2)
    firm = np.argwhere((out[k + "_lo"] == out[k + "_hi"]) & (dev[k][2] != 0)) if ref.bf16 else np.argwhere(dev[k][2] != 0)
    r, j = firm[len(firm) // 2]
    h = dev[k].copy()
    h[2, r, j] *= 1 + 2.0 ** -7
    with pytest.raises(AssertionError, match="step 2 " + k):
        dr.check_case(ref, {**dev, k: h}, tokens, parents)
