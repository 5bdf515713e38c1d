"""CPU: the sampled decode's pinned noise (tests/philox_ref.py against Philox4x32-10's known answers), the command line's sampling flags,
and the library's export of lrcn_sample_batch (no GPU call)."""
import importlib
import os
import subprocess
import sys

import numpy as np

import lrcn_amd  # noqa: F401
from lrcn_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import philox_ref as ph  # noqa: E402


def test_philox_known_answers():
    w = ph.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(x) for x in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    w = ph.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(x) for x in w] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_philox_vectorised_equals_scalar_and_seed_split():
    cols = np.arange(37)
    seed = 0x299F31D0A4093822
    g = ph.noise(seed, 5, 3, 7, cols)
    for c in (0, 1, 2, 3, 4, 17, 36):
        x = ph.philox4x32_10(c >> 2, 7, 3, 5, 0xA4093822, 0x299F31D0)[c & 3]
        assert g[c] == ph.gumbel(x)
    assert g.dtype == np.float32


def test_gumbel_range_is_finite_and_pinned():
    lo, hi = ph.gumbel(np.uint32(0)), ph.gumbel(np.uint32(0xFFFFFFFF))
    assert np.isfinite(lo) and np.isfinite(hi)
    assert abs(float(lo) + 2.812) < 1e-3 and abs(float(hi) - 16.636) < 1e-3
    # the pruning bound: a column more than PRUNE * T below the max never beats the max column's worst noise
    assert ph.PRUNE - (float(hi) - float(lo)) > 0.5


def test_draw_restatement_greedy_and_topk():
    z = np.array([0.5, 2.0, 2.0, -1.0, 1.5], np.float32)
    assert ph.draw(z, 0.0, 0, 1, 0, 0, 1) == 1            # greedy: lowest column of the tie
    assert list(ph.admitted(z, 2)) == [1, 2]
    assert list(ph.admitted(z, 3)) == [1, 2, 4]
    for seed in range(50):
        assert ph.draw(z, 1.0, 2, seed, 0, 0, 1) in (1, 2)


def _cli():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    return importlib.import_module("lrcn")


def test_cli_sampling_flags_and_defaults():
    cli = _cli()
    p = cli.build_parser()
    base = vars(p.parse_args([]))
    assert base["sample"] == 0 and base["temperature"] == 1.0 and base["topk"] == 0
    o = vars(p.parse_args(["--generate", "20", "--sample", "5", "--temperature", "0.8", "--topk", "10", "--seed", "7"]))
    assert (o["sample"], o["temperature"], o["topk"], o["seed"], o["generate"]) == (5, 0.8, 10, 7, 20)
    # the new flags leave every existing argument's default as it was
    for k, v in base.items():
        if k not in ("sample", "temperature", "topk"):
            assert vars(p.parse_args([]))[k] == v
    assert base["beam_width"] == 3 and base["seed"] == -1 and base["generate"] == 0


def test_sample_batch_is_exported_and_bound():
    assert "lrcn_sample_batch" in _lib.SAMPLE_SIGNATURES
    assert "lrcn_sample_batch" not in _lib.SIGNATURES   # include/lrcn.h (and the CPU oracle's ABI) stay as they are
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "lrcn_sample_batch" for line in out.splitlines())
    L = _lib.lib()
    assert L.lrcn_sample_batch.argtypes == _lib.SAMPLE_SIGNATURES["lrcn_sample_batch"][1]
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "lrcn_sample.h")).read()
    assert "int lrcn_sample_batch(" in hdr and '#include "lrcn.h"' in hdr


def test_stage_boundary_fixture_draws_the_last_column():
    """tests/stage_boundary.py, the fixture of test_gpu_sample.py::test_replay_f32_at_the_stage_boundary: at V = 15360 and 15361 and both
    draw settings, the last word holds between 0.1 and 0.5 of every row the host sampler reads, and the host draws it at least once."""
    import stage_boundary as sb
    assert sb.STAGE_V == (15360, 15361)
    for V in sb.STAGE_V:
        for T, top_k in sb.DRAWS:
            res = sb.host_samples(V, T, top_k)
            assert len(res) == sb.N * sb.S
            shares = [p for _, sh in res for p in sh]
            last = sum(int(t == V - 1) for seq, _ in res for t in seq[1:])
            print("V %d T %.1f top_k %d: p(V - 1) in [%.3f, %.3f], %d of %d host draws are column V - 1"
                  % (V, T, top_k, min(shares), max(shares), last, len(shares)))
            assert sb.LAST_SHARE[0] <= min(shares) and max(shares) <= sb.LAST_SHARE[1]
            assert last >= 1
