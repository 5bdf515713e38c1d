"""GPU: `tools/lrcn.py --train --varlen` on the tiny dataset of the existing driver tests: an epoch runs, a loss line is logged, no caption
is dropped where the reference's batcher drops its last window -- and on captions of mixed lengths."""
import importlib
import json
import os
import re
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt

from test_gpu_cli import _epoch_losses, _scene_dataset

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _cli():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    return importlib.import_module("lrcn")


def _dropped(out, split="train"):
    m = re.search(r"^%s: (\d+) captions, (\d+) dropped" % split, out, flags=re.M)
    assert m, out
    return int(m.group(1)), int(m.group(2))


def test_varlen_training_drops_no_caption(tmp_path, capsys):
    cli = _cli()
    tr, fp, _ = _scene_dataset(tmp_path)
    common = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "16", "--atype", "f32",
              "--seed", "3", "--train", "--lr", "0.01", "--dropout", "0.0"]
    ck = str(tmp_path / "v.npz")
    assert cli.main(common + ["--epochs", "4", "--varlen", "--savefile", ck]) == 0
    out = capsys.readouterr().out
    losses = _epoch_losses(out)
    assert len(losses) == 4 and len(losses[0]) == 2 and losses[-1][0] < losses[0][0], out
    assert _dropped(out) == (80, 0) and _dropped(out, "dev") == (80, 0)
    _, _, adam, _ = fmt.load_checkpoint(ck)
    assert adam["step"] == 4 * 5                      # 80 captions in windows of 16: every one of them trained on
    assert cli.main(common + ["--epochs", "1"]) == 0  # the default batcher: forced batch 10, the scan's last window goes
    n, lost = _dropped(capsys.readouterr().out)
    assert n == 80 and lost == 10


def test_varlen_training_on_mixed_lengths(tmp_path, capsys):
    cli = _cli()
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(36):
        a, b = img % 4, (img // 4) % 3
        f = np.zeros(4096, np.float32)
        f[a * 100:a * 100 + 50] = 1.0
        f[1000 + b * 100:1000 + b * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns.append({"image_id": img, "caption": "A %s %s ." % (nouns[a], verbs[b])})
        anns.append({"image_id": img, "caption": "The %s %s now ." % (nouns[a], verbs[b])})
        if img % 2:
            anns.append({"image_id": img, "caption": "One %s that %s all day ." % (nouns[a], verbs[b])})
    tr = str(tmp_path / "captions.json")
    with open(tr, "w") as fh:
        json.dump({"annotations": anns}, fh)
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)
    args = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "32", "--atype", "bf16",
            "--seed", "3", "--train", "--lr", "0.01", "--dropout", "0.0", "--epochs", "8", "--varlen"]
    assert cli.main(args) == 0
    out = capsys.readouterr().out
    losses = _epoch_losses(out)
    assert len(losses) == 8 and losses[-1][0] < 0.7 * losses[0][0], out
    assert _dropped(out) == (90, 0)
    assert re.search(r"3 batches of up to 32, \d+\.\d% of the rows are padding", out), out
