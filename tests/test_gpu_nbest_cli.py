"""GPU: tools/lrcn.py --generate --nbest: `nbest` holds --beam_width lines per image, best score first, and candidates / ids keep each image's
first line; without --nbest there is no nbest file."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_generate_with_nbest(tmp_path, capsys):
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
        return read("candidates.txt"), read("candidate_ids.txt"), read("nbest.txt")

    cands, ids, nbest = run("nb3", ["--nbest", "--beam_width", "3", "--length_norm", "1"])
    assert len(cands) == len(ids) == 12 and all(c.endswith(".") for c in cands)
    assert len(nbest) == 36
    by_id = {}
    for line in nbest:
        i, sc, lp, text = line.split("\t")
        by_id.setdefault(int(i), []).append((float(sc), float(lp), text))
    assert sorted(by_id) == sorted(int(i) for i in ids) and all(len(v) == 3 for v in by_id.values())
    for i, c in zip(ids, cands):
        entries = by_id[int(i)]
        assert [e[0] for e in entries] == sorted((e[0] for e in entries), reverse=True)   # best score first
        assert c == entries[0][2]
        for sc, lp, text in entries:
            assert sc >= lp - 1e-6   # logp <= 0 and len >= 1: the per-token score is not below the total
    plain = run("beam3", ["--beam_width", "3"])
    assert plain[2] is None and len(plain[0]) == 12
