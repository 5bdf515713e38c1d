"""GPU: tools/lrcn.py --generate --nbest --loadfile m0 --ensemble m1: two tiny checkpoints of different seeds and sizes decode together and
the `nbest` / `diverse` files keep their names and change; without --ensemble the ensemble call does not run and the files are what they
were; --ensemble without --nbest, checkpoints of different vocabularies, a wrong number of weights or a weight <= 0 are argparse errors."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt
from lrcn_amd import lrcn as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_generate_with_an_ensemble(tmp_path, capsys, monkeypatch):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]

    def corpus(name, nouns_):
        anns = []
        for img in range(48):
            anns.append({"image_id": img, "caption": "A %s %s ." % (nouns_[img % 4], verbs[(img // 4) % 3])})
        path = str(tmp_path / name)
        with open(path, "w") as fh:
            json.dump({"annotations": anns}, fh)
        return path

    feats = {}
    for img in range(48):
        a, b = img % 4, (img // 4) % 3
        f = np.zeros(4096, np.float32)
        f[a * 100:a * 100 + 50] = 1.0
        f[1000 + b * 100:1000 + b * 100 + 50] = 1.0
        feats[img] = f / f.sum()
    tr = corpus("captions.json", nouns)
    tr_other = corpus("captions_other.json", ["dog", "cat", "man", "fish"])   # the same number of words, another word list
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)

    def common(data, hidden, embed, seed):
        return ["--coco", "--datafiles", data, data, "--features", fp, fp, "--hidden", str(hidden), str(hidden), "--embed", str(embed),
                "--batchsize", "8", "--atype", "f32", "--seed", str(seed)]

    ck0, ck1, ck_other = str(tmp_path / "m0.npz"), str(tmp_path / "m1.npz"), str(tmp_path / "other.npz")
    train = ["--train", "--lr", "0.01", "--dropout", "0.0"]
    assert cli.main(common(tr, 64, 64, 3) + train + ["--epochs", "3", "--savefile", ck0]) == 0
    assert cli.main(common(tr, 32, 48, 4) + train + ["--epochs", "1", "--savefile", ck1]) == 0   # another seed, other sizes, less trained
    assert cli.main(common(tr_other, 32, 48, 4) + train + ["--epochs", "1", "--savefile", ck_other]) == 0
    capsys.readouterr()
    base = common(tr, 64, 64, 3)
    gen = ["--loadfile", ck0, "--generate", "4", "--capnumber", "12", "--nbest", "--beam_width", "2", "--length_norm", "1"]

    def run(name, extra):
        out = str(tmp_path / name)
        assert cli.main(base + gen + ["--out", out] + extra) == 0
        return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}

    def forbidden(*a, **k):
        raise AssertionError("the ensemble call ran without --ensemble")

    with monkeypatch.context() as mp:   # without --ensemble: the single-model entry points, as before
        mp.setattr(L, "beam_ensemble_batch", forbidden)
        plain = run("plain", [])
        groups = run("groups", ["--diverse_groups", "2"])
        assert run("plain2", ["--ensemble_mode", "logprob"]) == plain   # byte for byte: the mode alone selects nothing
    assert sorted(plain) == ["candidate_ids.txt", "candidates.txt", "nbest.txt"] and sorted(groups) == ["candidate_ids.txt", "candidates.txt", "diverse.txt"]
    ens = run("ens", ["--ensemble", ck1])
    assert sorted(ens) == sorted(plain) and ens["nbest.txt"] != plain["nbest.txt"]
    assert ens["candidate_ids.txt"] == plain["candidate_ids.txt"] and len(ens["nbest.txt"].decode().splitlines()) == 24
    assert ens["candidates.txt"].decode().splitlines() == [ln.split("\t")[3] for ln in ens["nbest.txt"].decode().splitlines()[::2]]
    weighted = run("weighted", ["--ensemble", ck1, "--ensemble_weights", "1,3", "--ensemble_mode", "logprob"])
    assert sorted(weighted) == sorted(plain) and weighted["nbest.txt"] not in (plain["nbest.txt"], ens["nbest.txt"])
    ensg = run("ensg", ["--ensemble", ck1, "--diverse_groups", "2", "--min_len", "3"])
    assert sorted(ensg) == sorted(groups) and ensg["diverse.txt"] != groups["diverse.txt"]
    for line in ensg["diverse.txt"].decode().splitlines():
        assert len([w for w in line.split("\t")[4].split() if w != "."]) >= 3, line   # --min_len through the ensemble
    three = run("three", ["--ensemble", ck1, ck0, "--ensemble_weights", "1,1,2"])
    assert sorted(three) == sorted(plain)
    capsys.readouterr()
    no_nbest = ["--loadfile", ck0, "--generate", "4", "--capnumber", "12", "--ensemble", ck1]
    for bad in (no_nbest, gen + ["--ensemble", ck_other], gen + ["--ensemble", ck1, "--ensemble_weights", "1"],
                gen + ["--ensemble", ck1, "--ensemble_weights", "1,2,3"], gen + ["--ensemble", ck1, "--ensemble_weights", "1,0"],
                gen + ["--ensemble", ck1, "--ensemble_weights", "1,-2"], gen + ["--ensemble_weights", "1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad + ["--out", str(tmp_path / "bad")])
        assert e.value.code == 2   # argparse's error exit
        assert "error:" in capsys.readouterr().err
