"""GPU: tools/lrcn.py --generate --nbest with --ban_words / --min_len / --no_repeat_ngram: the `nbest` file holds no banned word, no repeated
n-gram and no caption shorter than --min_len; without the flags the unconstrained call runs and the files are what they were; a word outside
the vocabulary, <eos>, or a flag without --nbest is an argparse error."""
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


def test_generate_with_constraints(tmp_path, capsys, monkeypatch):
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
    # the vocabulary has 11 words: 4 words per caption and 2 beams keep every constrained call feasible (V - nbanned - 1 - nword >= K)
    gen = ["--loadfile", ck, "--generate", "4", "--capnumber", "12", "--nbest", "--beam_width", "2", "--length_norm", "1"]

    def run(name, extra, args=gen):
        out = str(tmp_path / name)
        assert cli.main(common + args + ["--out", out] + extra) == 0
        return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}

    def forbidden(*a, **k):
        raise AssertionError("the constrained call ran without a constraint flag")

    with monkeypatch.context() as mp:   # without the flags: the unconstrained entry points, as before
        mp.setattr(L, "beam_constrained_batch", forbidden)
        plain = run("plain", [])
        groups = run("groups", ["--diverse_groups", "2"])
    assert sorted(plain) == ["candidate_ids.txt", "candidates.txt", "nbest.txt"] and sorted(groups) == ["candidate_ids.txt", "candidates.txt", "diverse.txt"]
    assert run("empty", ["--ban_words", "", "--min_len", "0", "--no_repeat_ngram", "0"]) == plain   # byte for byte
    words = [w for line in plain["nbest.txt"].decode().splitlines() for w in line.split("\t")[3].split() if w != "."]
    ban = sorted(set(words), key=lambda w: (-words.count(w), w))[:2]   # the two words the free lists use most

    def check(text, col):
        lines = text.decode().splitlines()
        assert len(lines) == 24
        for line in lines:
            cap = [w for w in line.split("\t")[col].split() if w != "."]
            assert not set(cap) & set(ban), line
            assert len(cap) >= 3, line                                  # --min_len (a truncated caption has all 4 words)
            grams = list(zip(cap, cap[1:]))
            assert len(grams) == len(set(grams)), line                  # --no_repeat_ngram 2

    flags = ["--ban_words", ",".join(ban), "--min_len", "3", "--no_repeat_ngram", "2"]
    con = run("con", flags)
    assert sorted(con) == sorted(plain) and con["nbest.txt"] != plain["nbest.txt"]
    check(con["nbest.txt"], 3)
    assert con["candidates.txt"].decode().splitlines() == [ln.split("\t")[3] for ln in con["nbest.txt"].decode().splitlines()[::2]]
    cong = run("cong", flags + ["--diverse_groups", "2"])
    assert sorted(cong) == sorted(groups)
    check(cong["diverse.txt"], 4)
    capsys.readouterr()
    for bad in (gen + ["--ban_words", "zeppelin"], gen + ["--ban_words", "<eos>"],
                ["--loadfile", ck, "--generate", "4", "--capnumber", "12", "--min_len", "2"],
                ["--loadfile", ck, "--generate", "4", "--capnumber", "12", "--ban_words", ban[0]],
                ["--loadfile", ck, "--generate", "4", "--capnumber", "12", "--no_repeat_ngram", "2"]):
        with pytest.raises(SystemExit) as e:
            cli.main(common + bad + ["--out", str(tmp_path / "bad")])
        assert e.value.code == 2   # argparse's error exit
        assert "error:" in capsys.readouterr().err
