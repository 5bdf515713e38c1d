"""GPU: tools/lrcn.py --generate --sample S: candidates / ids keep one line per image (the best of the S draws), `samples` holds all of
them; at temperature 0 one draw per image is beam search of width 1."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_generate_with_sampling(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(48):
        a, b = img % 4, (img // 4) % 3
        f = np.zeros(4096, np.float32)
        f[a * 100:a * 100 + 50] = 1.0
        f[1000 + b * 100:1000 + b * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns.append({"image_id": img, "caption": "A %s %s ." % (nouns[a], verbs[b])})
    tr = str(tmp_path / "captions.json")
    with open(tr, "w") as fh:
        json.dump({"annotations": anns}, fh)
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)
    ck = str(tmp_path / "m.npz")
    common = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "8",
              "--atype", "f32", "--seed", "3"]
    assert cli.main(common + ["--train", "--epochs", "3", "--lr", "0.01", "--savefile", ck, "--dropout", "0.0"]) == 0
    capsys.readouterr()

    def run(name, extra):
        out = str(tmp_path / name)
        assert cli.main(common + ["--loadfile", ck, "--generate", "20", "--capnumber", "12", "--out", out] + extra) == 0
        read = lambda f: open(os.path.join(out, f)).read().splitlines() if os.path.exists(os.path.join(out, f)) else None  # noqa: E731
        return read("candidates.txt"), read("candidate_ids.txt"), read("samples.txt")

    cands, ids, samples = run("s5", ["--sample", "5", "--temperature", "0.8"])
    assert len(cands) == len(ids) == 12 and all(c.endswith(".") for c in cands)
    assert len(samples) == 60
    by_id = {}
    for line in samples:
        i, lp, text = line.split("\t")
        by_id.setdefault(int(i), []).append((float(lp), text))
    assert sorted(by_id) == sorted(int(i) for i in ids) and all(len(v) == 5 for v in by_id.values())
    for i, c in zip(ids, cands):   # the candidate is the draw of highest log-likelihood
        best = max(by_id[int(i)], key=lambda t: t[0])
        assert c == best[1]
    again = run("s5b", ["--sample", "5", "--temperature", "0.8"])
    assert again == (cands, ids, samples)   # --seed fixes the draws
    # temperature 0, one draw per image == beam search of width 1; without --sample there is no samples file
    g = run("greedy", ["--sample", "1", "--temperature", "0"])
    b = run("beam1", ["--beam_width", "1"])
    assert g[0] == b[0] and g[1] == b[1] and b[2] is None
