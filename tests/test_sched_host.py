"""CPU: the host side of scheduled sampling (include/lrcn_sched.h) -- the coin's counter layout, the epsilon schedule, the wrapper's
argument checks, the reference with separate inputs and targets, and the seeded cases of tests/test_gpu_sched.py held to its caps in the
host simulation."""
import numpy as np
import pytest

from lrcn_amd import lrcn as L
from lrcn_amd import sched as S
from oracle import oracle as orc

import sched_ref as sr
import varlen_ref as vr
import weighted_ref as wr


def philox_int(c, k):
    """Philox4x32-10 in plain Python integers (Salmon et al., SC'11), written apart from tests/philox_ref.py's numpy form."""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_philox_known_answers():
    # the known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)
    assert philox_int([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert philox_int([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert philox_int([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_coin_counter_layout_and_the_map_to_u():
    # counter (0xFFFFFFFF, s, 0xFFFFFFFF, row0 + b), key (seed low, seed high), word 0; u = ((x >> 9) + 0.5) 2^-23 in float32
    for seed, s, row in [(2 ** 64 - 1, 0xFFFFFFFF, 0xFFFFFFFF), (7, 1, 0), (0x123456789ABCDEF0, 5, 1003), (3 << 32, 28, 2 ** 32 - 1)]:
        x = philox_int([0xFFFFFFFF, s, 0xFFFFFFFF, row], [seed & 0xFFFFFFFF, seed >> 32])[0]
        u = sr.coin_u(seed, s, [row])
        assert u.dtype == np.float32 and u[0] == np.float32((x >> 9) + 0.5) * np.float32(2.0 ** -23)
        assert np.float32(2.0 ** -24) <= u[0] <= np.float32(1.0 - 2.0 ** -24)
    assert sr.coin_u(2 ** 64 - 1, 0xFFFFFFFF, [0xFFFFFFFF])[0] == np.float32((0x408F276D >> 9) + 0.5) * np.float32(2.0 ** -23)
    # rows depend on row0 + b alone
    assert np.array_equal(sr.coin_u(9, 3, np.arange(1000, 1013)), sr.coin_u(9, 3, 1000 + np.arange(13)))
    lens = np.asarray([3, 0, 2, 3], np.int32)
    whole = sr.coins(11, 0.5, np.tile(lens, 2), 3, 0)
    assert np.array_equal(whole[:, 4:], sr.coins(11, 0.5, lens, 3, 4))
    # no coin at s = 0 or past a row's end; none fires below 2^-24, all fire at 1
    assert not whole[0].any() and not whole[1:, 1].any() and not whole[3, 2]
    assert not sr.coins(11, 1e-9, lens, 3, 0).any()
    assert sr.coins(11, 1.0, lens, 3, 0).sum() == lens.sum()
    # the coin rate over many rows is eps within four binomial standard deviations
    n = 20000
    rate = (sr.coin_u(5, 2, np.arange(n)) < np.float32(0.25)).mean()
    assert abs(rate - 0.25) <= 4 * np.sqrt(0.25 * 0.75 / n)


def test_epsilon_schedule():
    assert [S.epsilon(e, -1, 5, 0.05, 0.25) for e in (0, 3, 100)] == [0.0, 0.0, 0.0]
    assert [S.epsilon(e, 2, 5, 0.05, 0.25) for e in (0, 1)] == [0.0, 0.0]
    got = [S.epsilon(e, 2, 5, 0.05, 0.25) for e in (2, 6, 7, 11, 12, 22, 27, 500)]
    assert got == pytest.approx([0.05, 0.05, 0.10, 0.10, 0.15, 0.25, 0.25, 0.25])
    assert S.epsilon(1, 1, 1, 0.5, 0.5) == 0.5 and S.epsilon(0, 1, 1, 0.5, 0.5) == 0.0
    assert S.epsilon(3, 0, 1, 0.3, 1.0) == 1.0
    with pytest.raises(ValueError):
        S.epsilon(0, 0, 0, 0.05, 0.25)
    with pytest.raises(ValueError):
        S.epsilon(0, 0, 1, 0.05, 1.5)
    f = S.sched_of(1, 1, 0.5, 0.5, temperature=0.7, seed=3)
    assert f(0) is None
    eps, temp, seed = f(1)
    assert (eps, temp) == (0.5, 0.7) and 0 <= seed < 2 ** 64 and seed != f(2)[2]
    assert len({S.step_seed(seed, k) for k in range(100)}) == 100 and all(0 <= S.step_seed(seed, k) < 2 ** 64 for k in range(100))


def test_wrapper_rejects_bad_sched_arguments_before_any_call():
    for bad in [(float("nan"), 1.0, 0), (-0.1, 1.0, 0), (1.5, 1.0, 0), (0.5, float("nan"), 0), (0.5, -1.0, 0), (0.5, float("inf"), 0),
                (0.5, 1.0, 0, -1), (0.5, 1.0, 0, 2 ** 32 - 3), (0.5, 1.0, -1), (0.5, 1.0, 2 ** 64), (0.5, 1.0), (0.5,)]:
        with pytest.raises(L.LrcnError):
            L._sched(bad, 4)
    s = L._sched((0.5, 0.0, 2 ** 64 - 1, 2 ** 32 - 4), 4)
    assert (s.eps, s.temperature, s.seed, s.row0) == (0.5, 0.0, 2 ** 64 - 1, 2 ** 32 - 4)
    s = L._sched(L.Sched(0.25, seed=9), 4)
    assert (s.eps, s.temperature, s.seed, s.row0) == (0.25, 1.0, 9, 0)
    assert list(L._sched_lens(None, 5, 3)) == [5, 5, 5]


def test_reference_under_gold_inputs_is_the_padded_weighted_loss():
    B, T, E, H, V = 5, 4, 12, 8, 23
    rng = np.random.default_rng(3)
    for nl in (2, 1):
        m = orc.init_weights(E, H, H, V, seed=4, n_layers=nl)
        feats = (rng.standard_normal((B, 4096)) * 0.02).astype(np.float32)
        tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
        lens = np.asarray([4, 0, 2, 3, 1], np.int32)
        gold = sr.gold_inputs(tokens, lens)
        assert (gold[0] == 1).all() and gold[1, 1] == 0 and gold[3, 2] == 0 and gold[2, 2] == tokens[1, 2]
        ref, ref_g = vr.loss(m, feats, tokens, lens, 40, want_grad=True)
        val, g = sr.loss(m, feats, tokens, lens, gold, norm_tokens=40, want_grad=True)
        assert abs(val - ref) <= 1e-5 * abs(ref)
        for n in orc.PARAM_NAMES:
            if ref_g.p[n].size:
                np.testing.assert_allclose(g.p[n], ref_g.p[n], rtol=1e-3, atol=1e-5, err_msg=n)
        w = np.asarray([1.0, -0.5, 0.0, 2.0, 0.25], np.float32)
        refw = wr.loss(m, feats, tokens, lens, w, 40)
        assert abs(sr.loss(m, feats, tokens, lens, gold, norm_tokens=40, row_w=w) - refw) <= 1e-5 * abs(refw)
        # other inputs, another loss; the targets stay gold: a zero-weight row's targets do not matter
        fed = gold.copy()
        fed[2, 0] = (fed[2, 0] + 1) % V
        assert abs(sr.loss(m, feats, tokens, lens, fed, norm_tokens=40) - val) > 1e-9
        t2 = tokens.copy()
        t2[:, 2] = (t2[:, 2] + 5) % V
        assert sr.loss(m, feats, t2, lens, gold, norm_tokens=40, row_w=w) == sr.loss(m, feats, tokens, lens, gold, norm_tokens=40, row_w=w)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_seeded_cases_hold_enough_draws_and_few_near_ties(name):
    dtype, nl, B, T, E, H, V, eps, temp, row0, mixed, calls = sr.CASES[name]
    m, feats, tokens, lens, seeds = sr.case_inputs(name)
    assert len(seeds) == calls and (not mixed or (lens.min() == 0 and lens.max() == T))
    draws = near = 0
    for seed in seeds:
        fed, logits, fire, n = sr.simulate(m, feats, tokens, lens, eps, temp, seed, row0)
        assert fire.sum() <= lens.sum() and logits.shape == (T + 1, B, V)
        gold = sr.gold_inputs(tokens, lens)
        assert np.array_equal(fed[~fire], gold[~fire])
        draws += int(fire.sum())
        near += n
    print(name, "draws", draws, "near ties", near)
    assert draws >= sr.MIN_DRAWS
    assert near <= sr.EXCUSED_SHARE * draws
    if temp == 0:
        assert near == 0


def test_input_seeds_of_the_first_five_cases_are_their_old_ranks():
    first = ["bf16-B48-eps.5-t1", "f32-1layer-eps1-t1-row1000", "f32-V16400-eps1-t1", "f32-eps.5-t1", "f32-eps1-t0-row1000"]
    assert first == sorted(first) and [sr._INPUT_SEED[n] for n in first] == list(range(5))
    assert set(sr._INPUT_SEED) == set(sr.CASES) and len(set(sr._INPUT_SEED.values())) == len(sr.CASES)


@pytest.mark.parametrize("name", sr.LAST_COLUMN_CASES)
def test_last_column_cases_draw_the_last_column(name):
    """The cases on both sides of k_sched_next_input's staging boundary (and the unstaged bf16 one): the last word holds between 0.1 and
    0.5 of every logits row the draws read, and the host simulation draws it -- about a quarter of the case's draws."""
    dtype, nl, B, T, E, H, V, eps, temp, row0, mixed, calls = sr.CASES[name]
    m, feats, tokens, lens, seeds = sr.case_inputs(name)
    assert (V in (15360, 15361)) == (dtype == "f32") and eps == 1.0 and temp == 1.0
    lo, hi = sr.LAST_COLUMN_SHARE
    last = draws = 0
    for seed in seeds:
        fed, logits, fire, _ = sr.simulate(m, feats, tokens, lens, eps, temp, seed, row0)
        z = logits[:T].astype(np.float64)          # the rows of steps 0 .. T - 1 decide inputs 1 .. T
        p = np.exp(z - z.max(axis=2, keepdims=True))
        share = p[:, :, V - 1] / p.sum(axis=2)
        assert lo <= share.min() and share.max() <= hi, (name, share.min(), share.max())
        draws += int(fire.sum())
        last += int((fed[fire] == V - 1).sum())
    print(name, "draws", draws, "of column V - 1:", last)
    assert last >= 1 and draws >= sr.MIN_DRAWS
