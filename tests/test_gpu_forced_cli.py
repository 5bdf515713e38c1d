"""GPU: tools/lrcn.py --generate --nbest --force_words / --force_file: a tiny checkpoint decodes with words forced into every caption, the
`forced` file is written next to `candidates`, every written caption holds a word of each of its image's sets, and the options compose with
--ban_words / --min_len; a word outside the vocabulary, <eos>, more than 3 sets or 4 alternatives, and use with --diverse_groups or
--ensemble are argparse errors."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_generate_with_forced_words(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    adjs, advs = ["big", "small", "red", "old", "wet", "shy"], ["fast", "slowly", "today", "outside", "again", "there"]   # a vocabulary of 24
    anns, feats = [], {}
    for img in range(48):
        a, b = img % 4, (img // 4) % 3
        anns.append({"image_id": img, "caption": "A %s %s %s %s ." % (adjs[img % 6], nouns[a], verbs[b], advs[(img // 6) % 6])})
        f = np.zeros(4096, np.float32)
        f[a * 100:a * 100 + 50] = 1.0
        f[1000 + b * 100:1000 + b * 100 + 50] = 1.0
        feats[img] = f / f.sum()
    tr = str(tmp_path / "captions.json")
    with open(tr, "w") as fh:
        json.dump({"annotations": anns}, fh)
    fp = str(tmp_path / "feats.npz")
    fmt.save_features(fp, feats)
    base = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "8", "--atype", "f32",
            "--seed", "3"]
    ck = str(tmp_path / "m.npz")
    assert cli.main(base + ["--train", "--lr", "0.01", "--dropout", "0.0", "--epochs", "3", "--savefile", ck]) == 0
    capsys.readouterr()
    gen = ["--loadfile", ck, "--generate", "6", "--capnumber", "12", "--nbest", "--beam_width", "2", "--length_norm", "1"]

    def run(name, extra):
        out = str(tmp_path / name)
        assert cli.main(base + gen + ["--out", out] + extra) == 0
        return {f: open(os.path.join(out, f), "rb").read().decode() for f in sorted(os.listdir(out))}, capsys.readouterr().out

    def words_of(line):
        return [w for w in line.split("\t")[-1].split() if w != "."]

    plain, _ = run("plain", [])
    assert sorted(plain) == ["candidate_ids.txt", "candidates.txt", "nbest.txt"]
    # the same sets for every image: ("bird" or "cat") and "jumps"
    res, said = run("words", ["--force_words", "bird|cat,jumps"])
    assert sorted(res) == ["candidate_ids.txt", "candidates.txt", "forced.txt"]
    assert res["candidate_ids.txt"] == plain["candidate_ids.txt"] and res["forced.txt"] != plain["nbest.txt"]
    lines = res["forced.txt"].splitlines()
    assert len(lines) >= 12
    for ln in lines:
        w = words_of(ln)
        assert ("bird" in w or "cat" in w) and "jumps" in w, ln
    assert "forced words: 12 of 12 images with sets met them" in said
    first = {}
    for ln in lines:
        first.setdefault(ln.split("\t")[0], ln.split("\t")[3])
    ids = res["candidate_ids.txt"].split()
    assert res["candidates.txt"].splitlines() == [first[i] for i in ids]
    # composed with the negative constraints
    res2, _ = run("composed", ["--force_words", "bird|cat,jumps", "--ban_words", "man,big", "--min_len", "4", "--no_repeat_ngram", "1"])
    for ln in res2["forced.txt"].splitlines():
        w = words_of(ln)
        assert ("bird" in w or "cat" in w) and "jumps" in w and "man" not in w and "big" not in w and len(set(w)) == len(w), ln
        assert len(w) >= 4 or len(w) == 6, ln   # --min_len binds a caption that ends; one cut at --generate words has all 6
    # per image: two images with sets of their own, the others free
    ff = str(tmp_path / "force.txt")
    with open(ff, "w") as fh:
        fh.write("%s man,sleeps\n%s\tdog|cat|bird|man\n" % (ids[0], ids[1]))
    res3, said = run("file", ["--force_file", ff])
    assert sorted(res3) == sorted(res) and "forced words: 2 of 2 images with sets met them" in said
    by_image = {}
    for ln in res3["forced.txt"].splitlines():
        by_image.setdefault(ln.split("\t")[0], []).append(ln)
    for ln in by_image[ids[0]]:
        assert "man" in words_of(ln) and "sleeps" in words_of(ln), ln
    for ln in by_image[ids[1]]:
        assert set(words_of(ln)) & {"dog", "cat", "bird", "man"}, ln
    plain_by_image = {}
    for ln in plain["nbest.txt"].splitlines():
        plain_by_image.setdefault(ln.split("\t")[0], []).append(ln.split("\t")[3])
    for i in ids[2:]:   # an image without a line: its n-best captions
        assert [ln.split("\t")[3] for ln in by_image[i]] == plain_by_image[i], i
    capsys.readouterr()
    for bad in (gen + ["--force_words", "zebra"], gen + ["--force_words", "<eos>"], gen + ["--force_words", "dog,cat,man,bird"],
                gen + ["--force_words", "dog|cat|man|bird|runs"], gen + ["--force_words", "dog", "--diverse_groups", "2"],
                gen + ["--force_words", "dog", "--ensemble", ck], gen + ["--force_words", "dog", "--ban_words", "dog"],
                gen + ["--force_words", "dog|dog"], gen + ["--force_words", "dog", "--force_file", ff],
                ["--loadfile", ck, "--generate", "6", "--capnumber", "12", "--force_words", "dog"],
                ["--loadfile", ck, "--generate", "6", "--capnumber", "12", "--nbest", "--beam_width", "16", "--force_words", "dog,cat"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad + ["--out", str(tmp_path / "bad")])
        assert e.value.code == 2, bad   # argparse's error exit
        assert "error:" in capsys.readouterr().err
