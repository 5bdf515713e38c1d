"""CPU: the nucleus / any-top_k selection's host restatement (tests/nucleus_ref.py) on hand-checked cases, the command line's --topp and
--topk, the library's export of the entry points of include/lrcn_nucleus.h, and the self-checks of the fixtures that the GPU tests
(tests/test_gpu_nucleus.py) stand on -- a bad fixture fails here, without a GPU."""
import importlib
import os
import subprocess
import sys

import numpy as np

import lrcn_amd  # noqa: F401
from lrcn_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nucleus_ref as nr  # noqa: E402
import philox_ref as ph  # noqa: E402


# ------------------------------------------------------------------------------------------------ 1. hand-checked cases
def test_hand_checked_sizes():
    z = np.log(np.array([0.15, 0.5, 0.05, 0.3], np.float64)).astype(np.float32)   # shares 0.5, 0.3, 0.15, 0.05 in scrambled columns
    assert list(nr.rank_order(z)) == [1, 3, 0, 2]
    assert nr.nucleus_size(z, 1.0, 0, 0.79)[0] == 2
    assert nr.nucleus_size(z, 1.0, 0, 0.81)[0] == 3
    assert nr.nucleus_size(z, 1.0, 0, 1.0)[0] == 4
    assert list(nr.admitted(z, 1.0, 0, 0.79)) == [1, 3]
    # top_k = 2: renormalised to 0.625, 0.375 -- 0.7 needs both
    n, G = nr.nucleus_size(z, 1.0, 2, 0.7)
    assert n == 2 and np.allclose(G, [0.0, 0.625, 1.0])
    assert nr.nucleus_size(z, 1.0, 2, 0.6)[0] == 1
    # temperature: z / T with T = 0.5 squares the shares (0.25, 0.09, 0.0225, 0.0025 of 0.365): the top word alone holds 0.68
    assert nr.nucleus_size(z, 0.5, 0, 0.6)[0] == 1 and nr.nucleus_size(z, 0.5, 0, 0.7)[0] == 2


def test_boundary_tie_enters_by_lower_column():
    z = np.array([1.0, 3.0, 1.0, 1.0, 0.0], np.float32)
    assert list(nr.rank_order(z)) == [1, 0, 2, 3, 4]
    e = np.exp(np.array([0.0, -2.0, -2.0, -2.0, -3.0]))
    G = np.cumsum(e) / e.sum()
    p = float(0.5 * (G[1] + G[2]))          # needs two of the three tied columns
    n, _ = nr.nucleus_size(z, 1.0, 0, p)
    assert n == 3 and list(nr.admitted(z, 1.0, 0, p)) == [0, 1, 2]
    assert list(nr.admitted(z, 1.0, 3, 1.0)) == [0, 1, 2] and list(nr.admitted(z, 1.0, 2, 1.0)) == [0, 1]
    # -0 and +0 are one value: column order decides
    zz = np.array([0.0, -0.0, 1.0], np.float32)
    assert list(nr.rank_order(zz)) == [2, 0, 1]
    for seed in range(40):
        assert nr.draw(z, 1.0, 0, p, seed, 0, 0, 1) in (0, 1, 2)
        assert nr.draw(z, 1.0, 3, 1.0, seed, 0, 0, 1) == ph.draw(z, 1.0, 3, seed, 0, 0, 1)


# ------------------------------------------------------------------------------------------------ 2. command line
def _tool(name):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    return importlib.import_module(name)


def test_cli_topp_and_wide_topk():
    p = _tool("lrcn").build_parser()
    base = vars(p.parse_args([]))
    assert base["topp"] == 1.0 and base["topk"] == 0 and base["sample"] == 0 and base["temperature"] == 1.0
    assert base["beam_width"] == 3 and base["seed"] == -1 and base["generate"] == 0
    o = vars(p.parse_args(["--generate", "20", "--sample", "5", "--topp", "0.9", "--topk", "100"]))
    assert (o["topp"], o["topk"], o["sample"], o["generate"]) == (0.9, 100, 5, 20)
    for k, v in base.items():   # the new flag moves no other default
        if k not in ("topp", "topk", "sample", "generate"):
            assert o[k] == v, k


# ------------------------------------------------------------------------------------------------ 3. exports
def test_nucleus_entry_points_are_exported_and_bound():
    names = ("lrcn_sample_batch_p", "lrcn_sample_logits")
    assert set(_lib.NUCLEUS_SIGNATURES) == set(names)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "lrcn_nucleus.h")).read()
    assert '#include "lrcn.h"' in hdr
    L = _lib.lib()
    for n in names:
        assert n in exported
        assert n not in _lib.SIGNATURES and n not in _lib.SAMPLE_SIGNATURES
        assert "int %s(" % n in hdr
        assert getattr(L, n).argtypes == _lib.NUCLEUS_SIGNATURES[n][1]
    assert "lrcn_sample_batch_p" not in open(os.path.join(os.path.dirname(HERE), "include", "lrcn.h")).read()


# ------------------------------------------------------------------------------------------------ 4. fixture self-checks
def test_decisive_fixture_gaps_and_excused_draws():
    """Every decisive row holds its intended size with every prefix share >= 6e-3 from top_p (asserted in the builders), covers n* = 1, 2,
    10..60 and n* = V at V = 37 with every share >= 0.012, and fewer than 1 % of the host draws are near-ties."""
    draws = exc = 0
    for V in nr.DECISIVE_V:
        for T in nr.DECISIVE_T:
            cases = nr.decisive_cases(V, T)
            assert [c[2] for c in cases] == nr.n_stars(V)
            for z, top_p, n in cases:
                assert z.shape == (V,) and z.dtype == np.float32 and 0.0 < top_p < 1.0
                assert nr.nucleus_size(z, T, 0, top_p)[0] == n
            for toks, ex in nr.decisive_host_draws(V, T):
                draws += len(toks)
                exc += int(ex.sum())
    z37 = nr.decisive_cases(37, 1.0)[-1][0]
    sh = np.exp(z37.astype(np.float64))
    assert (sh / sh.sum()).min() >= nr.MIN_SHARE and nr.decisive_cases(37, 1.0)[-1][2] == 37
    print("decisive fixture: %d of %d host draws excused" % (exc, draws))
    assert exc < 0.01 * draws, (exc, draws)


def test_stage_boundary_rows_put_their_mass_in_the_last_column():
    """V = 15360 | 15361, the last staged and the first unstaged width of k_sample_nucleus: every decisive row's largest share is column
    V - 1, and at each (V, T) the host draws that column -- all S draws of the n* = 1 row, which admits nothing else, and some of the wider
    rows'.  A device copy of the row that stops at V - 1 cannot give these draws."""
    assert set(nr.STAGE_BOUNDARY_V) <= set(nr.DECISIVE_V) and nr.STAGE_BOUNDARY_V == (15360, 15361)
    for V in nr.STAGE_BOUNDARY_V:
        for T in nr.DECISIVE_T:
            last = 0
            for (z, top_p, n), (toks, ex) in zip(nr.decisive_cases(V, T), nr.decisive_host_draws(V, T)):
                assert int(np.argmax(z)) == V - 1 and (z[:V - 1] < z[V - 1]).all()
                if n == 1:
                    assert (toks == V - 1).all() and not ex.any()
                last += int((toks == V - 1).sum())
            print("V %d T %.1f: %d host draws of column V - 1" % (V, T, last))
            assert last >= nr.DECISIVE_S


def test_tie_and_combination_fixtures():
    for V in (203, 10640):
        rng = np.random.default_rng([V, 7])
        z, top_p, n, tcols = nr.tie_row_top_p(V, 1.0, rng)
        adm = nr.admitted(z, 1.0, 0, top_p)
        assert n == 8 and list(np.intersect1d(adm, tcols)) == list(tcols[:3])   # the three LOWEST of the eight tied columns
        z, k, tcols = nr.tie_row_top_k(V, 1.0, rng)
        adm = ph.admitted(z, k)
        assert list(np.intersect1d(adm, tcols)) == list(tcols[:5])
        assert list(adm) == list(nr.admitted(z, 1.0, k, 1.0))
        for n_star in nr.COMBO_N:
            z, n = nr.combo_row(V, 0.7, n_star, rng)
            assert nr.nucleus_size(z, 0.7, 50, 0.9)[0] == n_star
            assert nr.nucleus_size(z, 0.7, 0, 0.9)[0] > 50      # without the cut the nucleus would be wider: the renormalisation matters


def test_natural_rows_span_small_and_large_nuclei():
    rows = nr.natural_rows(10640, 5)
    sizes = [nr.nucleus_size(z, T, 0, p)[0] for z in rows for T in (0.7, 1.0, 1.5) for p in (0.5, 0.9, 0.99)]
    assert min(sizes) <= 10 and max(sizes) >= 1000, (min(sizes), max(sizes))


def test_production_fixture_has_judged_rows():
    """The structural bf16 test judges a row if the bf16-emulating oracle gives its top word a share >= 0.1 at every step of the greedy
    caption, and needs at least half of its sampled rows judged.  Here: every fourth of those rows, on the oracle's own greedy captions."""
    m = nr.production_model()
    rows = nr.production_rows()[::4]
    f = np.stack([nr.production_feats()[r // nr.PROD_S] for r in rows])
    caps = nr.oracle_greedy(m, f, 8)
    jd = nr.judged(m, f, caps)
    print("%d of %d rows judged" % (int(jd.sum()), len(rows)))
    assert jd.sum() >= 0.5 * len(rows)
