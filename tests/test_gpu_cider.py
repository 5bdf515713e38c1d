"""GPU: CIDEr-D on the device (include/lrcn_cider.h, lrcn_amd/cider_device.py) against lrcn_amd.cider.CiderD over the same ids written as
word strings: a hand-made corpus with every edge named, seeded corpora at V = 13 and V = 70 001, the fixed summation order, the argument
errors, and scst.scst_step / tools/lrcn.py --scst_reward device against the host reward.

Tolerance: |device - host| <= 1e-12 * max(1, |host|), and exactly 0.0 where the host gives exactly 0.0.  Every term is non-negative, the idf
values are the host's bits, and what differs is the order of sums of at most about 250 terms and one exp / sqrt per reference: a few hundred
units of 1.1e-16, under 1e-13; 1e-12 leaves a factor of ten.

The hand-made corpus comes in two forms of 6 images and V = 40, because two of its cases exclude each other: a word in EVERY image's
references (idf exactly 0) needs every image to have references, and "an image without references" needs one that has none.  Form A has
the common word in all six images; form B is form A with image 5's references taken away.  An empty hypothesis is out_len = 2 with eos;
out_len = 1 is below the [2, ld] every row has (bos and at least one step) and is one of the refused arguments below."""
import ctypes as C
import functools
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch

import lrcn_amd
from lrcn_amd import _lib, dp, scst
from lrcn_amd import captions as cap
from lrcn_amd import formats as fmt
from lrcn_amd import lrcn as L
from lrcn_amd import train as trn
from lrcn_amd.cider import CiderD
from lrcn_amd.cider_device import DeviceCiderD

import cider_cases as cc

pytestmark = pytest.mark.gpu
F32 = lrcn_amd.LRCN_F32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(dev, host, names=None):
    dev, host = np.asarray(dev, np.float64), np.asarray(host, np.float64)
    assert dev.shape == host.shape
    for k, (d, h) in enumerate(zip(dev, host)):
        name = names[k] if names else k
        if h == 0.0:
            assert d == 0.0, (name, d)
        else:
            assert abs(d - h) <= 1e-12 * max(1.0, abs(h)), (name, d, h, d - h)


def device_metric(refs, V):
    return DeviceCiderD({i: [cc.as_words(r) for r in rs] for i, rs in refs.items()}, cc.identity_vocab(V), 2)


# ------------------------------------------------------------------------------------------------ 1. the hand-made corpus
HAND_V = 40
COMMON = 3      # in every image's references of form A: df = N, idf exactly 0
HAND_A = {
    0: [[3, 4, 5, 6, 7, 8]],                                                                                      # one reference
    1: [[3, 9, 10, 11], [3, 9, 10, 12, 13], [9, 10, 11, 3], [14, 3, 15], [3, 16, 17, 18, 19, 20, 21], [9, 9, 3, 10]],   # six
    2: [[3, 22, 22, 23], [3, 24]],                                                                                # 22 twice; a reference shorter than n = 3
    3: [[3], [3, 25, 26, 27, 28]],                                                                                # a one-word reference
    4: [[3, 29, 30, 31, 32, 33], [], ([3, 29, 30, 31, 32, 33, 31] * 36)[:250]],                                   # an empty reference; a long one
    5: [[3, 34, 35, 36], [34, 35, 36, 3, 37]],
}
HAND_B = dict(HAND_A)
HAND_B[5] = []                                                                                                    # an image without references
LONG = ([3, 29, 30, 31, 32, 33, 30] * 37)[:256]     # (against a short reference the length penalty underflows to 0: image 4 has a long one)
# name -> (form, image, words, closing eos, junk behind out_len)
HAND_CASES = {
    "equal to its reference": ("A", 0, [3, 4, 5, 6, 7, 8], True, None),
    "equal to one of six references": ("A", 1, [3, 9, 10, 12, 13], True, None),
    "shares no n-gram with its image": ("A", 0, [38, 39, 38], True, None),
    "another image's reference": ("A", 0, [3, 25, 26, 27, 28], True, None),
    "empty (out_len 2, eos)": ("A", 1, [], True, None),
    "one word": ("A", 3, [25], True, None),
    "two words": ("A", 3, [3, 25], True, None),
    "three words": ("A", 3, [3, 25, 26], True, None),
    "six times a word the reference has twice": ("A", 2, [22] * 6, True, None),
    "only the common word: 1-gram norm 0": ("A", 3, [3], True, None),
    "the common word three times": ("A", 3, [3, 3, 3], True, None),
    "n-grams in no reference": ("A", 1, [3, 9, 38, 39, 10, 11], True, None),
    "against a reference shorter than n": ("A", 2, [3, 24], True, None),
    "against an empty reference": ("A", 4, [3, 29, 30, 31], True, None),
    "256 words": ("A", 4, LONG, True, None),
    "256 words, no eos": ("A", 4, LONG, False, None),
    "ends without eos": ("A", 5, [34, 35, 36, 3], False, None),
    "junk behind out_len": ("A", 5, [3, 34, 35, 36], True, 35),
    "junk behind out_len, no eos": ("A", 5, [34, 35, 36, 3, 37], False, 3),
    "image without references": ("B", 5, [3, 34, 35, 36], True, None),
    "form B: the common word now has idf > 0": ("B", 3, [3], True, None),
    "form B: equal to its reference": ("B", 0, [3, 4, 5, 6, 7, 8], True, None),
}


def test_hand_made_corpus():
    ld = 258
    for form, refs in (("A", HAND_A), ("B", HAND_B)):
        host = cc.host_metric(refs)
        dev = device_metric(refs, HAND_V)
        names = [n for n, c in HAND_CASES.items() if c[0] == form]
        rows, lens, want = [], [], []
        for n in names:
            _, img, words, eos, junk = HAND_CASES[n]
            t, ol = cc.pack([words], ld=ld, eos=eos, junk=junk)
            rows.append(t[0])
            lens.append(ol[0])
            want.append(host.score(img, cc.as_words(words)))
        got = dev.score_ids([HAND_CASES[n][1] for n in names], np.stack(rows), np.asarray(lens))
        for n, g, w in zip(names, got, want):
            print("%-45s device %.17g host %.17g" % (n, g, w))
        check(got, want, names)
        w = dict(zip(names, want))
        st = dev.stats()
        if form == "A":
            assert host.idf((str(COMMON),)) == 0.0
            assert w["equal to its reference"] > 5.0 and w["shares no n-gram with its image"] == 0.0 and w["empty (out_len 2, eos)"] == 0.0
            assert w["only the common word: 1-gram norm 0"] == 0.0 and w["the common word three times"] == 0.0
            assert 0.0 < w["six times a word the reference has twice"] < w["one word"] and w["256 words"] > 0.0 and w["ends without eos"] > 0.0
            assert w["junk behind out_len"] == host.score(5, cc.as_words([3, 34, 35, 36])) > 0.0
            assert st["images"] == 6 and st["references"] == 16 and st["ngrams"][0] == len(host._idf[0]) and st["ngrams"][3] == len(host._idf[3])
        else:
            assert w["image without references"] == 0.0 and w["form B: the common word now has idf > 0"] > 0.0 and st["references"] == 14
        assert all(s >= 2 * g and s & (s - 1) == 0 for s, g in zip(st["slots"], st["ngrams"])) and st["device_bytes"] > 0
        dev.close()


# ------------------------------------------------------------------------------------------------ 2. seeded corpora
@functools.lru_cache(maxsize=None)
def seeded_device(V):
    return device_metric(cc.seeded(V)[0], V)


@functools.lru_cache(maxsize=None)
def seeded_rows(V):
    hyps = cc.seeded(V)[1]
    tok, out_len = cc.pack([h for _, h in hyps])
    return [i for i, _ in hyps], tok, out_len


@pytest.mark.parametrize("V", [13, 70001])
def test_seeded_corpus(V):
    host = cc.seeded_host_scores(V)
    assert len(host) == 300
    pos, zero = float((host > 0).mean()), float((host == 0).mean())
    print("V=%d: share of host scores above 0 %.3f, exact zeros %.3f" % (V, pos, zero))
    if V == 13:
        assert pos >= 0.9
    else:
        assert pos >= 0.3 and zero >= 0.6
    ids, tok, out_len = seeded_rows(V)
    got = seeded_device(V).score_ids(ids, tok, out_len)
    print("V=%d: largest |device - host| %.3g (largest host score %.4f)" % (V, float(np.abs(got - host).max()), float(host.max())))
    check(got, host)
    # score_batch and corpus pack the same rows
    assert np.array_equal(seeded_device(V).score_batch(ids[:9], [h for _, h in cc.seeded(V)[1][:9]]), got[:9])
    mean, per = seeded_device(V).corpus({ids[0]: cc.seeded(V)[1][0][1]})
    assert per == {ids[0]: got[0]} and mean == got[0]


# ------------------------------------------------------------------------------------------------ 3. the fixed order
def test_scores_do_not_depend_on_the_batch():
    V = 13
    dev = seeded_device(V)
    ids, tok, out_len = seeded_rows(V)
    a = dev.score_ids(ids, tok, out_len)
    b = dev.score_ids(ids, tok, out_len)
    assert np.array_equal(a, b)
    rev = dev.score_ids(ids[::-1], tok[::-1], out_len[::-1])
    assert np.array_equal(rev[::-1], a)
    for k in range(0, 300, 15):      # 20 hypotheses, each alone
        alone = dev.score_ids(ids[k:k + 1], tok[k:k + 1], out_len[k:k + 1])
        assert alone[0] == a[k], (k, alone[0], a[k])
    # the device-pointer form: the same kernel on the caller's arrays, queued on the handle's stream
    index = torch.as_tensor(np.asarray([dev.index_of[i] for i in ids], np.int32)).cuda()
    out = dev.score_rows_dev(index, torch.as_tensor(tok).cuda(), torch.as_tensor(out_len).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), a)


def test_device_form_contract_rows():
    """lrcn_cider_score_dev checks no row on the host: a row with a bad image index or length gets a NaN and reads no table; an id outside
    [0, V) is no index, it only matches no reference word."""
    dev = device_metric(HAND_A, HAND_V)
    tok, out_len = cc.pack([[3, 4, 5, 6], [3, 4, 5, 6], [3, 4, 5, 6], [3, 4, 5, 6], [3, 4, 10 ** 6, 6], [3, 4, -5, 6], [3, 4, 38, 6]], ld=8)
    out_len[1], out_len[2] = 1, 9
    index = np.asarray([0, 0, 0, 6, 0, 0, 0], np.int32)
    got = dev.score_rows_dev(torch.as_tensor(index).cuda(), torch.as_tensor(tok).cuda(), torch.as_tensor(out_len).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = dev.score_batch([0, 0], [[3, 4, 5, 6], [3, 4, 38, 6]])       # 38 is in no reference either
    assert got[0] == want[0] > 0.0 and np.isnan(got[1:4]).all()
    assert got[4] == got[5] == got[6] == want[1] > 0.0
    dev.close()


# ------------------------------------------------------------------------------------------------ 4. errors
def test_bad_arguments_are_refused_before_any_work():
    dev = device_metric(HAND_A, HAND_V)
    lib = _lib.lib()
    good_tok, good_len = cc.pack([[3, 4, 5], [3, 9, 10], [3, 22]], ld=8)
    good_img = np.asarray([0, 1, 2], np.int32)
    long_tok, long_len = cc.pack([[3], [3], [4] * 257], ld=260)

    def call(tok, out_len, img, R, ld=None, null=None):
        out = np.full(3, -7.5, np.float64)
        p = {"tokens": tok.ctypes.data_as(C.POINTER(C.c_int32)), "out_len": out_len.ctypes.data_as(C.POINTER(C.c_int32)),
             "image": img.ctypes.data_as(C.POINTER(C.c_int32)), "out": out.ctypes.data_as(C.POINTER(C.c_double))}
        if null:
            p[null] = None
        rc = lib.lrcn_cider_score(dev._h, p["tokens"], tok.shape[1] if ld is None else ld, p["out_len"], p["image"], R, p["out"])
        assert np.array_equal(out, np.full(3, -7.5)), "the output array was written"
        return rc, lib.lrcn_cider_last_error(dev._h).decode()

    def changed(a, r, c, v):
        a = a.copy()
        if c is None:
            a[r] = v
        else:
            a[r, c] = v
        return a

    for null in ("tokens", "out_len", "image", "out"):
        rc, msg = call(good_tok, good_len, good_img, 3, null=null)
        assert rc == -1 and "null" in msg, (null, rc, msg)
    rc, msg = call(good_tok, good_len, good_img, 0)
    assert rc == -1 and "R=0" in msg
    cases = {
        "image below 0": (good_tok, good_len, changed(good_img, 1, None, -1), "row 1"),
        "image at n_images": (good_tok, good_len, changed(good_img, 2, None, 6), "row 2"),
        "out_len 1": (good_tok, changed(good_len, 0, None, 1), good_img, "row 0"),
        "out_len above ld": (good_tok, changed(good_len, 2, None, 9), good_img, "row 2"),
        "257 words": (long_tok, long_len, good_img, "row 2"),
        "a word id of V": (changed(good_tok, 1, 2, HAND_V), good_len, good_img, "row 1"),
        "a negative word id": (changed(good_tok, 2, 1, -1), good_len, good_img, "row 2"),
    }
    for name, (tok, out_len, img, row) in cases.items():
        rc, msg = call(np.ascontiguousarray(tok), out_len, img, 3)
        assert rc == -1 and row in msg, (name, rc, msg)
    # junk behind out_len is not a word: ids out of range there are not looked at
    tok = good_tok.copy()
    tok[0, good_len[0]:] = 10 ** 6
    assert np.array_equal(dev.score_rows(good_img, tok, good_len), dev.score_rows(good_img, good_tok, good_len))
    with pytest.raises(lrcn_amd.LrcnError, match="no references in this DeviceCiderD"):
        dev.score_batch([77], [[3]])
    with pytest.raises(lrcn_amd.LrcnError, match="row 0"):
        dev.score_batch([0], [[3, HAND_V + 5]])
    dev.close()


# ------------------------------------------------------------------------------------------------ 5. through scst_step
E = H = 64
NWORD = 6
MAX_B = 96


@functools.lru_cache(maxsize=None)
def scene():
    """The "scene" corpus of tests/test_gpu_scst.py, rebuilt: 48 images whose feature vector names a noun and a verb.
    -> (annotations, caps, vocab, padded blocks of 12, feature table, references by image, id -> word)."""
    nouns, verbs = ["dog", "cat", "man", "bird"], ["runs", "sleeps", "jumps"]
    anns, feats = [], {}
    for img in range(48):
        n, v = nouns[img % 4], verbs[(img // 4) % 3]
        f = np.zeros(4096, np.float32)
        f[(img % 4) * 100:(img % 4) * 100 + 50] = 1.0
        f[1000 + ((img // 4) % 3) * 100:1000 + ((img // 4) % 3) * 100 + 50] = 1.0
        feats[img] = f / f.sum()
        anns.append({"image_id": img, "caption": "A %s %s ." % (n, v)})
        anns.append({"image_id": img, "caption": "The %s %s now ." % (n, v)})
        if img % 3 == 0:
            anns.append({"image_id": img, "caption": "A %s ." % n})
    caps = cap.tokenize_coco(json.dumps({"annotations": anns}))
    vocab = cap.build_vocab([caps], threshold=1)
    return anns, caps, vocab, cap.minibatch_varlen(caps, vocab, 12), feats, scst.references_by_image(caps, vocab), cap.index_to_word(vocab)


def feats_of(ids):
    return L.to_jl(np.stack([scene()[4][i] for i in ids]).astype(np.float32))


def new_ctx():
    ctx = L.Context(E, H, H, len(scene()[2]), max_B=MAX_B, max_T=NWORD + 1, lstm_dtype=F32)
    ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    return ctx


@functools.lru_cache(maxsize=None)
def pretrained():
    """The nine parameter arrays after three epochs of cross-entropy on the scene corpus (deterministic context: the same bits every time)."""
    blocks = list(scene()[3])
    ctx = new_ctx()
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    optim.lr = 0.01
    tr = dp.DataParallelTrainer(ctx, param, optim, 12, 1, 0, pdrop=0.0, seed=7)
    hist = trn.train(tr, [blocks], 3, seed=3, feats_of=feats_of, log=lambda s: None, sync=ctx.sync)
    assert hist[-1][0] < hist[0][0]
    out = [L.from_jl(p).copy() for p in param]
    tr.close()
    ctx.close()
    return out


def make_trainer(ctx):
    param = L.model_from_arrays(pretrained())
    optim = L.initparams(param)
    optim.lr = 1e-3
    return dp.DataParallelTrainer(ctx, param, optim, 16, 1, 0, pdrop=0.0, seed=7), param


def scene_device_metric():
    _, _, vocab, _, _, refs, _ = scene()
    word_ids = {w: i - 1 for w, i in vocab.items()}      # the C ABI's ids
    return DeviceCiderD(refs, word_ids, word_ids[cap.UNK_WORD])


class Counting:
    """A reward object: score_batch only, counting its calls and keeping what it was asked."""

    def __init__(self, inner):
        self.inner, self.calls, self.asked = inner, 0, []

    def score_batch(self, image_ids, id_lists):
        self.calls += 1
        self.asked += [(i, [int(t) for t in w]) for i, w in zip(image_ids, id_lists)]
        return self.inner.score_batch(image_ids, id_lists)


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_scst_step_with_the_device_reward(baseline):
    _, _, _, _, _, refs, idx2word = scene()
    ids, S, seed = [0, 5, 10, 15], 4, 5
    host_reward = scst.cider_reward(CiderD(refs), idx2word)
    asked = []

    def recording(image_id, words):
        asked.append((image_id, [int(t) for t in words]))
        return host_reward(image_id, words)

    ctx = new_ctx()
    tr_h, _ = make_trainer(ctx)
    out_h = scst.scst_step(tr_h, feats_of(ids), ids, recording, S, NWORD, seed=seed, baseline=baseline)
    ctx.sync()
    tr_h.close()
    counting = Counting(scene_device_metric())
    tr_d, _ = make_trainer(ctx)
    out_d = scst.scst_step(tr_d, feats_of(ids), ids, counting, S, NWORD, seed=seed, baseline=baseline)
    ctx.sync()
    tr_d.close()
    print("scst_step, %s baseline: host %s | device %s" % (baseline, out_h, out_d))
    assert counting.calls == (2 if baseline == "greedy" else 1)          # one call for the N S samples, one for the N greedy captions
    assert counting.asked == asked and len(asked) == len(ids) * S + (len(ids) if baseline == "greedy" else 0)   # the same samples, in the same order
    assert abs(out_d["reward_sample"] - out_h["reward_sample"]) <= 1e-12 and out_h["reward_sample"] > 0.0
    if baseline == "greedy":
        assert abs(out_d["reward_greedy"] - out_h["reward_greedy"]) <= 1e-12      # (this model's greedy captions of these images score 0.0 on the host)
    else:
        assert out_d["reward_greedy"] is None and out_h["reward_greedy"] is None
    assert out_d["stepped"] == out_h["stepped"] is True and out_d["zero_share"] == out_h["zero_share"]
    assert abs(out_d["loss"] - out_h["loss"]) <= 1e-6 * abs(out_h["loss"]), (out_d["loss"], out_h["loss"])
    counting.inner.close()
    ctx.close()


def test_beam_cider_with_the_device_metric():
    _, _, _, _, _, refs, idx2word = scene()
    ctx = new_ctx()
    param = L.model_from_arrays(pretrained())
    ids = list(range(12))
    counting = Counting(scene_device_metric())
    want = scst.beam_cider(ctx, param, CiderD(refs), ids, feats_of, idx2word, 3, NWORD, chunk=5)
    got = scst.beam_cider(ctx, param, counting, ids, feats_of, idx2word, 3, NWORD, chunk=5)
    assert counting.calls == 1 and len(counting.asked) == 12
    print("beam_cider: host %.17g device %.17g" % (want, got))
    assert abs(got - want) <= 1e-12 * max(1.0, want), (got, want)
    host = CiderD(refs)
    check(counting.inner.score_batch([i for i, _ in counting.asked], [w for _, w in counting.asked]),
          [host.score(i, [idx2word[t] for t in w]) for i, w in counting.asked])
    counting.inner.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ 8. the command line
def test_cli_scst_reward_device(tmp_path, capsys, monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    cli = importlib.import_module("lrcn")
    anns, _, vocab, _, feats, _, _ = scene()
    tr_json, va_json = str(tmp_path / "captions_train.json"), str(tmp_path / "captions_val.json")
    with open(tr_json, "w") as fh:
        json.dump({"annotations": anns}, fh)
    with open(va_json, "w") as fh:
        json.dump({"annotations": [a for a in anns if a["image_id"] < 12]}, fh)
    fp, ck = str(tmp_path / "feats.npz"), str(tmp_path / "ce.npz")
    fmt.save_features(fp, feats)
    fmt.save_checkpoint(ck, pretrained(), vocab)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    steps = []
    real_step = scst.scst_step

    def recording_step(*a, **kw):
        out = real_step(*a, **kw)
        steps.append(out)
        return out

    monkeypatch.setattr(scst, "scst_step", recording_step)
    argv = ["--coco", "--datafiles", tr_json, va_json, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "16",
            "--atype", "f32", "--seed", "3", "--train", "--scst", "--scst_samples", "4", "--scst_nword", "6", "--epochs", "1", "--lr", "0.001",
            "--dropout", "0.0", "--loadfile", ck]
    first, lines = {}, {}
    for where in ("device", "host"):
        del steps[:]
        assert cli.main(argv + ["--scst_reward", where]) == 0
        out = capsys.readouterr().out
        lines[where] = [ln for ln in out.splitlines() if ln.startswith("(:epoch, 1, :scst_reward, ")]
        assert len(lines[where]) == 1 and ":greedy_reward, " in lines[where][0] and ":dev_cider, " in lines[where][0], out[-2000:]
        assert len(steps) == 12          # 48 images, 4 per step
        first[where] = steps[0]
    print(lines)
    assert first["host"]["reward_sample"] > 0.0 and first["host"]["reward_greedy"] >= 0.0
    assert abs(first["device"]["reward_sample"] - first["host"]["reward_sample"]) <= 1e-12
    assert abs(first["device"]["reward_greedy"] - first["host"]["reward_greedy"]) <= 1e-12
    dev_cider = {w: float(lines[w][0].split(":dev_cider, ")[1].split(")")[0]) for w in lines}
    assert dev_cider["device"] >= 0.0 and dev_cider["host"] >= 0.0
    # outside --scst the flag is an error, as --ss_start is
    with pytest.raises(SystemExit, match="--scst_reward"):
        cli.main([a for a in argv if a != "--scst"] + ["--scst_reward", "device"])
