"""GPU: tools/lrcn.py --generate --nbest --diverse_groups: `diverse` holds --beam_width lines per image, grouped and best score first within
each group, candidates / ids keep the best-scoring entry over all groups; without --diverse_groups the outputs are the n-best ones, byte for
byte, and there is no diverse file."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

from lrcn_amd import formats as fmt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_generate_with_diverse_groups(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]   # the fixture of test_gpu_nbest_cli.py
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
        return {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}

    K, G = 6, 3
    res = run("dv", ["--nbest", "--beam_width", str(K), "--length_norm", "1", "--diverse_groups", str(G), "--diverse_strength", "1.5"])
    assert sorted(res) == ["candidate_ids.txt", "candidates.txt", "diverse.txt"]
    cands, ids = res["candidates.txt"].decode().splitlines(), res["candidate_ids.txt"].decode().splitlines()
    lines = res["diverse.txt"].decode().splitlines()
    assert len(cands) == len(ids) == 12 and len(lines) == 12 * K
    by_id = {}
    for line in lines:
        i, g, sc, lp, text = line.split("\t")
        by_id.setdefault(int(i), []).append((int(g), float(sc), float(lp), text))
    assert list(by_id) == [int(i) for i in ids]   # images in the order of the ids file, an image's lines together
    for i, c in zip(ids, cands):
        entries = by_id[int(i)]
        assert [e[0] for e in entries] == [g for g in range(G) for _ in range(K // G)]   # grouped, the groups in order
        for g in range(G):
            scores = [e[1] for e in entries if e[0] == g]
            assert scores == sorted(scores, reverse=True)   # best first within the group
        top = max(e[1] for e in entries)
        assert c in [e[3] for e in entries if e[1] == top]   # the best score over all groups (the file rounds scores to 6 places)
        for _, sc, lp, text in entries:
            assert sc >= lp - 1e-6 and text.endswith(".")
        assert len({e[3] for e in entries}) > K // G   # the groups do not all repeat one list
    # without --diverse_groups: today's n-best outputs, and two runs of it are byte-identical
    plain = run("nb", ["--nbest", "--beam_width", str(K), "--length_norm", "1"])
    again = run("nb2", ["--nbest", "--beam_width", str(K), "--length_norm", "1", "--diverse_strength", "1.5"])
    assert sorted(plain) == ["candidate_ids.txt", "candidates.txt", "nbest.txt"] and plain == again
    for line in plain["nbest.txt"].decode().splitlines():
        assert len(line.split("\t")) == 4
    # one group is the n-best list: the same captions, scores and candidates through the diverse path
    one = run("dv1", ["--nbest", "--beam_width", str(K), "--length_norm", "1", "--diverse_groups", "1"])
    assert one["candidates.txt"] == plain["candidates.txt"] and one["candidate_ids.txt"] == plain["candidate_ids.txt"]
    assert [ln.split("\t", 2)[2] for ln in one["diverse.txt"].decode().splitlines()] == [ln.split("\t", 1)[1] for ln in plain["nbest.txt"].decode().splitlines()]
