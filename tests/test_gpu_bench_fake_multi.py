"""GPU: `bench.py --gpus 2` end to end on ONE GPU (LRCN_BENCH_FAKE_MULTI=1: both ranks share device 0 and the process group is gloo -- RCCL
refuses two ranks per device), i.e. the launcher, the per-rank supervisors of the first-contact ladder, the N-rank control flow of dp.py
(row shards, global normaliser, per-group [event -> all-reduce -> fused Adam] pipeline on a probed update stream, sparse exchange of the
embedding gradient) and the step-1 self-check, all on the REAL kernels with only the transport swapped.  A validation, never a measurement:
the line says so in its metric.  (tests/test_bench_launcher.py drives every rung of the ladder with injected failures on the CPU.)
Also bench.py --dump-outputs end to end on one GPU."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_on_one_gpu_walk_the_ladder_and_pass_the_self_check():
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["LRCN_BENCH_FAKE_MULTI"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("VALIDATION") and d["n_gpus"] == 2 and d["value"] > 0
    rc = d["rccl"]
    assert rc["world"] == 2 and rc["mode"] == "default" and rc["rung"] == "1 of 2" and rc["fallback_reason"] is None
    assert rc["pipeline"]["per_group_pipeline"] and rc["pipeline"]["sparse_embedding_exchange"] and rc["pipeline"]["update_stream_on_its_own_queue"] is not None
    sc = rc["selfcheck"]
    assert sc["violations"] == []
    assert sc["world_from_communicator"] == 2 == sc["world_measured_by_allreduce"]
    assert sc["loss_rel_diff"] <= 1e-5 and sc["sparse_vs_dense_embed_grad_rel"] <= 1e-4
    assert sc["params_identical_before_step_1"] and sc["params_identical_after_warmup"] and sc["params_identical_after_last_step"]
    assert 3.0 < d["config"]["last_loss"] < 9.3   # below ln V = 9.27 after six steps on the two alternating batches, and finite


def test_dump_outputs_are_the_last_timed_step_and_reproducible(tmp_path):
    """bench.py --dump-outputs on a small one-GPU configuration: loss.npy is the line's last_loss and the nine parameters are written in their
    logical shapes; a second run with the same arguments writes the same bits (the timed path sums in a fixed order); and a run without the
    untimed sub-report pass -- which trains 8 more steps after the timed region -- writes the same bits as well, so the dump is the last
    TIMED step's."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from lrcn_amd import lrcn as L
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--spinup-ms", "0",
            "--hidden", "64", "--vocab", "300", "--T", "5", "--global-batch", "8"]

    def run(name, **extra):
        env = dict(os.environ)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LRCN_DETERMINISTIC"):
            env.pop(k, None)
        env.update(extra)
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--dump-outputs", str(d)],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        return line, {f[:-4]: np.load(d / f) for f in os.listdir(d)}

    la, a = run("a")
    assert la["steps"] == 3 and la["config"]["deterministic"] is True
    assert set(a) == {"loss", *L.PARAM_NAMES}
    assert a["loss"].dtype == np.float64 and a["loss"][0] == la["config"]["last_loss"]
    assert {n: a[n].shape for n in L.PARAM_NAMES} == dict(zip(L.PARAM_NAMES, map(tuple, L.param_shapes(64, 64, 64, 300))))   # all whole
    assert all(a[n].dtype == np.float32 for n in L.PARAM_NAMES)
    assert la["dump_outputs"]["shapes"] == {k: list(v.shape) for k, v in a.items()}
    lb, b = run("b")
    lc, c = run("c", LRCN_BENCH_SUBREPORTS="0")
    assert la["roofline"]["sub"] is not None and lc["roofline"]["sub"] is None
    for n in a:
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
        np.testing.assert_array_equal(a[n], c[n], err_msg=n)
