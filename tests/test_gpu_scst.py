"""GPU: self-critical caption training (lrcn_amd/scst.py) -- scst_step against the hand-written composition of its parts and against
tests/weighted_ref.py, the no-step rule for all-zero advantages, the reward it trains on going up, and tools/lrcn.py --train --scst.

The fixture is the "scene" corpus of tests/test_gpu_varlen.py (rebuilt here): 48 images whose feature vector names a noun and a verb, and
captions of three lengths that the image decides ("a dog runs", "the dog runs now", "a dog")."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import _lib, dp, scst
from lrcn_amd import captions as cap
from lrcn_amd import formats as fmt
from lrcn_amd import lrcn as L
from lrcn_amd import train as trn
from lrcn_amd.cider import CiderD
from oracle import oracle as orc

import weighted_ref as wr

pytestmark = pytest.mark.gpu
F32 = lrcn_amd.LRCN_F32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = H = 64
NWORD = 6                       # sampled captions: at most 6 words, so T <= 7
MAX_B = 96                      # the evaluation draw: 12 images x 8 samples

# The reward test's step count and margin: measured once on an MI355X, profiles/scst_bench.md "The reward test" (see the test's docstring)
SCST_STEPS = 40
SCST_MARGIN = 0.069     # half of the measured gain 0.6264 -> 0.7640


@functools.lru_cache(maxsize=None)
def scene():
    """-> (annotations, caps, vocab, padded blocks of 12, feature table, CiderD over the captions, id -> word)."""
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
    cider = CiderD(scst.references_by_image(caps, vocab))
    return anns, caps, vocab, cap.minibatch_varlen(caps, vocab, 12), feats, cider, cap.index_to_word(vocab)


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


def host(ts):
    return [L.from_jl(t).copy() for t in ts]


def make_trainer(ctx, lr=1e-3, gclip=0.0):
    param = L.model_from_arrays(pretrained())
    optim = L.initparams(param)
    optim.lr = lr
    return dp.DataParallelTrainer(ctx, param, optim, 16, 1, 0, pdrop=0.0, seed=7, gclip=gclip), param, optim


def test_scst_step_is_its_parts(monkeypatch):
    # the fused and the unfused Adam kernels agree to a last bit, not bit for bit (tests/test_gpu_fused_update.py): the trainer runs the
    # plain update here, as the composition below does
    monkeypatch.setenv("LRCN_FUSED_UPDATE", "0")
    _, _, vocab, _, _, cider, idx2word = scene()
    N, S, seed = 4, 4, 5
    ids = [0, 5, 10, 15]
    reward = scst.cider_reward(cider, idx2word)
    ctx = new_ctx()
    tr, pa, oa = make_trainer(ctx)
    out = scst.scst_step(tr, feats_of(ids), ids, reward, S, NWORD, seed=seed)
    ctx.sync()
    assert out["stepped"] and oa.t == 1 and 0.0 <= out["zero_share"] < 1.0
    got = host(pa)
    tr.close()

    # by hand: sample_batch, beam_search_batch with K = 1, CiderD, advantages, build_batch, lossgradient(row_weights=), update
    pb = L.model_from_arrays(pretrained())
    ob = L.initparams(pb)
    ob.lr = 1e-3
    f = feats_of(ids)
    samples = L.sample_batch(ctx, pb, f, S, NWORD, temperature=1.0, seed=seed)
    greedy = L.beam_search_batch(ctx, pb, f, 1, NWORD)
    words = lambda seq: [idx2word[t] for t in seq[1:] if t != L.EOS]     # noqa: E731  (eos can only close a row)
    r_s = [[cider.score(ids[i], words(seq)) for seq, _ in samples[i]] for i in range(N)]
    r_g = [cider.score(ids[i], words(seq)) for i, (seq, _) in enumerate(greedy)]
    adv = scst.advantages(r_s, r_g, "greedy")
    tok, out_len = scst.pack_samples(samples, NWORD)
    tokens, lens, w, nt = scst.build_batch(tok, out_len, adv)
    assert tokens.shape[1] == N * S and nt == int(lens.sum()) + N * S and np.count_nonzero(w) > 0
    rows = np.repeat(np.stack([scene()[4][i] for i in ids]), S, axis=0).astype(np.float32)
    grads, val = L.lossgradient(ctx, pb, L.to_jl(rows), tokens, lens=lens, norm_tokens=nt, row_weights=w)
    print("scst parts: rewards", np.mean(r_s), np.mean(r_g), "loss", val, "step's", out)
    assert abs(out["reward_sample"] - np.mean(r_s)) < 1e-12 and abs(out["reward_greedy"] - np.mean(r_g)) < 1e-12
    assert out["loss"] == val and out["zero_share"] == 1.0 - np.count_nonzero(w) / float(N * S)
    # the f32 gradient of the composition against the reference, on the sampled captions (tests/test_gpu_varlen.py's tolerances)
    model = orc.Model(E, H, H, len(vocab), arrays=dict(zip(orc.PARAM_NAMES, pretrained())))
    ref, ref_g = wr.loss(model, rows, tokens, lens, w, nt, want_grad=True)
    assert abs(val - ref) <= 1e-5 * abs(ref), (val, ref)
    for n, g in zip(orc.PARAM_NAMES, grads):
        np.testing.assert_allclose(L.from_jl(g), ref_g.p[n], rtol=1e-3, atol=1e-5, err_msg=n)
    L.update(ctx, pb, grads, ob)
    ctx.sync()
    for k, (a, b) in enumerate(zip(got, host(pb))):
        assert np.array_equal(a, b), "parameter %d: scst_step differs from its parts" % k
    assert any(np.abs(a - p0).max() > 0 for a, p0 in zip(got, pretrained()))
    # N S rows must fit the context
    with pytest.raises(lrcn_amd.LrcnError, match="max_B"):
        scst.scst_step(make_trainer(ctx)[0], feats_of(list(range(13))), list(range(13)), reward, 8, NWORD, seed=1)
    ctx.close()


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_all_zero_advantages_take_no_step(baseline):
    ctx = new_ctx()
    tr, param, optim = make_trainer(ctx)
    before = host(param)
    ids = [1, 2, 3]
    out = scst.scst_step(tr, feats_of(ids), ids, lambda image_id, words: 0.75, 4, NWORD, seed=2, baseline=baseline)
    ctx.sync()
    assert not out["stepped"] and out["loss"] is None and out["zero_share"] == 1.0 and out["reward_sample"] == 0.75
    assert out["reward_greedy"] == (0.75 if baseline == "greedy" else None)
    assert optim.t == 0 and tr.step_no == 0
    for a, b in zip(before, host(param)):
        assert np.array_equal(a, b)
    tr.close()
    ctx.close()


EVAL_IDS = list(range(12))      # every noun x verb pair once
EVAL_SEED, EVAL_S = 123, 8


def evaluate(ctx, param):
    """(mean CIDEr-D of a fixed draw -- seed 123, 8 samples per image, temperature 1 -- and of the greedy captions) over EVAL_IDS."""
    _, _, _, _, _, cider, idx2word = scene()
    reward = scst.cider_reward(cider, idx2word)
    f = feats_of(EVAL_IDS)
    tok, n = scst.pack_samples(L.sample_batch(ctx, param, f, EVAL_S, NWORD, temperature=1.0, seed=EVAL_SEED), NWORD)
    r_s = np.mean([reward(i, scst.sample_words(tok[k, s], n[k, s])) for k, i in enumerate(EVAL_IDS) for s in range(EVAL_S)])
    r_g = np.mean([reward(i, scst.sample_words(seq, len(seq))) for i, (seq, _) in zip(EVAL_IDS, L.beam_search_batch(ctx, param, f, 1, NWORD))])
    return float(r_s), float(r_g)


def run_scst(ctx, tr, steps, first=0):
    """`steps` scst_steps of 12 images x 4 samples, walking over the 48 images; step k draws with seed 1000 + k."""
    _, _, _, _, _, cider, idx2word = scene()
    reward = scst.cider_reward(cider, idx2word)
    for k in range(first, first + steps):
        ids = [(12 * k + j) % 48 for j in range(12)]
        scst.scst_step(tr, feats_of(ids), ids, reward, 4, NWORD, seed=1000 + k)


def test_scst_raises_the_reward_it_trains_on():
    """Cross-entropy for three epochs, then SCST_STEPS self-critical steps (12 images x 4 samples, Adam at 1e-3, CIDEr-D against the scene
    captions): the mean reward of a fixed evaluation draw must rise by more than SCST_MARGIN and the greedy captions' must not fall by
    more than that.  Both comparisons are against the same model before the steps, on a deterministic context.  K and the margin (half
    the gain measured at that K) are in profiles/scst_bench.md, "The reward test"."""
    ctx = new_ctx()
    tr, param, optim = make_trainer(ctx)
    s0, g0 = evaluate(ctx, param)
    run_scst(ctx, tr, SCST_STEPS)
    s1, g1 = evaluate(ctx, param)
    print("scst reward: K=%d sampled %.4f -> %.4f, greedy %.4f -> %.4f, margin %.4f" % (SCST_STEPS, s0, s1, g0, g1, SCST_MARGIN))
    assert optim.t > 0
    assert s1 > s0 + SCST_MARGIN
    assert g1 >= g0 - SCST_MARGIN
    tr.close()
    ctx.close()


def test_cli_train_scst(tmp_path):
    anns, _, vocab, _, feats, _, _ = scene()
    tr_json, va_json = str(tmp_path / "captions_train.json"), str(tmp_path / "captions_val.json")
    with open(tr_json, "w") as fh:
        json.dump({"annotations": anns}, fh)
    with open(va_json, "w") as fh:
        json.dump({"annotations": [a for a in anns if a["image_id"] < 12]}, fh)
    fp, ck, out = str(tmp_path / "feats.npz"), str(tmp_path / "ce.npz"), str(tmp_path / "scst.npz")
    fmt.save_features(fp, feats)
    fmt.save_checkpoint(ck, pretrained(), vocab)
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    argv = [sys.executable, os.path.join(ROOT, "tools", "lrcn.py"), "--coco", "--datafiles", tr_json, va_json, "--features", fp, fp, "--hidden", "64", "64",
            "--embed", "64", "--batchsize", "16", "--atype", "f32", "--seed", "3", "--train", "--scst", "--scst_samples", "4", "--scst_nword", "6",
            "--epochs", "2", "--lr", "0.001", "--dropout", "0.0", "--gclip", "5"]
    r = subprocess.run(argv + ["--loadfile", ck, "--savefile", out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("(:epoch, ")]
    assert len(lines) == 2, r.stdout[-2000:]
    for k, ln in enumerate(lines):
        assert ln.startswith("(:epoch, %d, :scst_reward, " % (k + 1)) and ":greedy_reward, " in ln and ":dev_cider, " in ln, ln
        vals = ln[ln.index("(") + 1:ln.index(")")].split(", ")
        assert all(float(vals[j]) >= 0.0 for j in (3, 5, 7)), ln
    model, vocab2, adam, _ = fmt.load_checkpoint(out)
    assert vocab2 == vocab and 0 < adam["step"] <= 2 * 12 and len(model) == 9   # 48 images / 4 per step; a step of all-zero advantages is not taken
    assert any(np.abs(np.asarray(a) - b).max() > 0 for a, b in zip(model, pretrained()) if b.size)
    # without a trained model to start from: a message, and a non-zero exit
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--loadfile" in r.stderr, (r.returncode, r.stderr[-500:])
