"""GPU: tools/lrcn_activity.py --train with --drop_in / --drop_out on a small feature file: a seeded run repeats bit for bit, differs from the
run without the flags, and the run without the flags is the plain training loop.

The parent's output for the same command: the flags' defaults send every step to ActivityModel.train_step's plain call, which this test
holds to a loop written against train_step's earlier signature (no dropout argument reaches it: lrcn_act_loss_grad, whose launches are
unchanged).  Beyond that, the command of `no_flags` below was run once on this tree and on its parent's checkout (own build of each) on the
same feature file: every array of the two checkpoints was equal (the new one holds the additional key drop_seed)."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def write_features(path, n_videos=6, F=64, seed=0):
    """What --extfeatures writes (n_videos, labels, names, video_i [n_frames x F]), with standardised random features whose class shows in
    the first two columns."""
    rng = np.random.default_rng(seed)
    out = {"n_videos": np.array(n_videos), "labels": np.array([v % 2 for v in range(n_videos)], np.int32),
           "names": np.array(["v%d" % v for v in range(n_videos)])}
    for v in range(n_videos):
        f = rng.standard_normal((int(rng.integers(5, 9)), F)).astype(np.float32)
        f[:, v % 2] += 2.0
        out["video_%d" % v] = f
    np.savez(path, **out)


def test_train_with_dropout_flags(tmp_path, capsys):
    from lrcn_amd import activity as A

    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn_activity")
    feats = str(tmp_path / "feats.npz")
    write_features(feats)
    base = ["--train", "--features", feats, "--hidden", "32", "--clip", "4", "--stride", "2", "--batchsize", "8", "--epochs", "3",
            "--lr", "0.01", "--seed", "2"]

    def run(name, extra):
        ck = str(tmp_path / name)
        assert cli.main(base + ["--savefile", ck] + extra) == 0
        return np.load(ck)

    drop = ["--drop_in", "0.5", "--drop_out", "0.5"]
    a, b, no_flags = run("a.npz", drop), run("b.npz", drop), run("c.npz", [])
    capsys.readouterr()
    assert set(a.files) == set(b.files) == set(no_flags.files) and "drop_seed" in a.files
    for k in a.files:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert int(a["drop_seed"]) == 2
    for n in A.PARAM_NAMES:
        assert not np.array_equal(a[n], no_flags[n]), n

    # the run without the flags = the plain loop (train() of the tool, with train_step as it was called before the flags existed)
    vf, labels, _ = cli.load_features(feats)
    m = A.ActivityModel(64, 32, 2, max_B=8, max_T=4, dtype=A.LRCN_BF16, seed=2)
    specs = [(v, s, n) for v, f in enumerate(vf) for (s, n) in A.clips(f.shape[0], 4, 2)]
    rng = np.random.default_rng(2)
    for _ in range(3):
        order = rng.permutation(len(specs))
        for i in range(0, len(order), 8):
            sp = [specs[k] for k in order[i:i + 8]]
            x, lens = A.gather_clips(vf, sp, 4)
            m.train_step(x, labels[[v for v, _, _ in sp]], lens, 4, lr=0.01, gclip=0.0)
    m.sync()
    ck = str(tmp_path / "loop.npz")
    m.save(ck)
    loop = np.load(ck)
    for k in loop.files:
        np.testing.assert_array_equal(loop[k], no_flags[k], err_msg=k)
    m.close()
