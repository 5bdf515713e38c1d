"""GPU: `tools/lrcn.py --train --label_smoothing E`, run as a child process on the tiny caption dataset of the other driver tests: with
--varlen it trains, logs finite epoch lines and saves a model; with E = 0 it is the run without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt

from test_gpu_cli import _epoch_losses, _scene_dataset

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CLI = os.path.join(os.path.dirname(HERE), "tools", "lrcn.py")


def run(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, CLI] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_label_smoothing_trains_and_zero_is_the_run_without_the_flag(tmp_path):
    tr, fp, _ = _scene_dataset(tmp_path)
    common = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "16", "--atype", "f32",
              "--seed", "3", "--train", "--epochs", "2", "--lr", "0.01", "--dropout", "0.0", "--varlen"]
    ck = str(tmp_path / "s.npz")
    out = run(common + ["--label_smoothing", "0.1", "--savefile", ck])
    smooth = _epoch_losses(out)
    assert len(smooth) == 2 and len(smooth[0]) == 2 and np.isfinite(smooth).all(), out
    model, vocab, adam, _ = fmt.load_checkpoint(ck)
    assert adam["step"] == 2 * 5 and all(np.isfinite(np.asarray(t)).all() for t in model)   # 80 captions in windows of 16, two epochs
    zero = _epoch_losses(run(common + ["--label_smoothing", "0"]))
    none = _epoch_losses(run(common))
    # the lines print four decimals and the loss sums are not ordered without LRCN_OPT_DETERMINISTIC: one unit of the last place
    assert len(zero) == len(none) == 2
    assert np.abs(np.asarray(zero) - np.asarray(none)).max() <= 1.0001e-4, (zero, none)
    # the epoch lines are average_loss's plain NLL of a model that was trained on another objective: they moved by far more than that
    assert np.abs(np.asarray(smooth) - np.asarray(none)).max() > 1e-3, (smooth, none)

