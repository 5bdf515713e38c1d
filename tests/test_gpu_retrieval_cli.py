"""GPU: tools/lrcn.py --retrieval (paper section 5.1 / Table 2) on a tiny model trained on 12 distinct noun x verb images: the two metric
lines, retrieval.json, scores.npy, and caption-to-image R@1 far above chance."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt
from lrcn_amd import retrieval

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def parse(line, head):
    assert line.startswith(head + ": "), line
    w = line[len(head) + 2:].split()
    return {w[k]: float(w[k + 1]) for k in range(0, len(w), 2)}


def test_retrieval_cli(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(12):   # 12 distinct images, each seen with its caption 4 times per epoch
        a, b = img % 4, img // 4
        f = np.zeros(4096, np.float32)
        f[a * 100:a * 100 + 50] = 1.0
        f[1000 + b * 100:1000 + b * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns += [{"image_id": img, "caption": "A %s %s ." % (nouns[a], verbs[b])}] * 4
    tr = str(tmp_path / "captions.json")
    with open(tr, "w") as fh:
        json.dump({"annotations": anns}, fh)
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)
    ck = str(tmp_path / "m.npz")
    common = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "8",
              "--atype", "f32", "--seed", "3"]
    assert cli.main(common + ["--train", "--epochs", "10", "--lr", "0.01", "--savefile", ck, "--dropout", "0.0"]) == 0
    capsys.readouterr()
    out = str(tmp_path / "ret")
    assert cli.main(common + ["--loadfile", ck, "--retrieval", "--capnumber", "12", "--out", out]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("Caption to Image", "Image to Caption"))]
    assert len(lines) == 2
    c2i, i2c = parse(lines[0], "Caption to Image"), parse(lines[1], "Image to Caption")
    assert sorted(c2i) == sorted(i2c) == ["Medr", "R@1", "R@10", "R@5"]
    with open(os.path.join(out, "retrieval.json")) as fh:
        js = json.load(fh)
    assert js["norm"] == "mean" and sorted(js["image_ids"]) == list(range(12)) and js["captions"] == 48
    s = np.load(os.path.join(out, "scores.npy"))
    assert s.shape == (12, 48) and np.isfinite(s).all() and (s < 0).all()
    again = retrieval.metrics(s, js["img_of_caption"], norm="mean", lens=js["lens"])
    for key, printed in (("caption_to_image", c2i), ("image_to_caption", i2c)):
        assert js[key] == again[key]
        for k, v in printed.items():
            assert abs(v - again[key][k]) <= 0.05 + 1e-9, (key, k, v, again[key][k])
    assert c2i["R@1"] >= 50.0, c2i   # chance is 1/12
    # the sum normalisation ranks images identically (same scores per caption)
    out2 = str(tmp_path / "ret_sum")
    assert cli.main(common + ["--loadfile", ck, "--retrieval", "--retrieval_norm", "sum", "--capnumber", "12", "--out", out2]) == 0
    with open(os.path.join(out2, "retrieval.json")) as fh:
        js2 = json.load(fh)
    assert js2["norm"] == "sum" and js2["caption_to_image"] == js["caption_to_image"]
