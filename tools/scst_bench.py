"""Self-critical caption training (lrcn_amd/scst.py, include/lrcn_weighted.h) on one GPU at the benchmark's caption shape (E = H = 1000,
V = 10640, bf16):

  split  one SCST step of N images x S samples, timed piece by piece, each piece ending in a host wait: the sampled decode
         (lrcn.sample_batch), the greedy decode (lrcn.beam_search_batch, K = 1), the rewards on the host (cider.CiderD on synthetic
         references: five per image, lengths from the COCO reference captions' histogram), and the weighted training step.  The model is
         freshly initialised, so nearly every sample runs to the length limit: the longest batch the step can meet.
  step   lrcn_train_step_w with every weight 1, and with every second weight 0, against lrcn_train_step_var on the same padded batch
         (lengths from the same histogram), alternated in one process; the spread of the lrcn_train_step_var rounds is printed beside them.

Prints one line per measurement and a JSON summary line.
--reward device runs the split's rewards with cider_device.DeviceCiderD (include/lrcn_cider.h) instead; --reward both runs the host and the
device reward in turn in every round on the same captions (one more row in the split) and reports the largest absolute difference between them.

usage: python tools/scst_bench.py [--images 64] [--samples 4] [--nword 20] [--rounds 5] [--steps 30] [--reward host|device|both] [--split_only]
                                  [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import lrcn_amd
from lrcn_amd import dp, scst
from lrcn_amd import lrcn as L
from lrcn_amd.cider import CiderD

E = H = 1000
V = 10640
# word counts of the 5000 COCO reference captions of the evaluation set (the fixture the host tests check the batcher on)
with open(os.path.join(ROOT, "tests", "golden", "coco_ref_caption_lengths.json")) as _fh:
    HIST = {int(k): v for k, v in json.load(_fh)["histogram"].items()}


def hist_lengths(n, rng, cap_at):
    ks = np.asarray(sorted(HIST))
    p = np.asarray([HIST[k] for k in ks], np.float64)
    return np.minimum(rng.choice(ks, size=n, p=p / p.sum()), cap_at).astype(np.int32)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def step_split(N, S, nword, rounds, rng, reward_mode="host"):
    ctx = L.Context(E, H, H, V, max_B=N * S, max_T=nword + 1, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    tr = dp.DataParallelTrainer(ctx, param, optim, N * S, 1, 0, pdrop=0.4, seed=1)
    words = ["w%d" % k for k in range(V)]
    ids = list(range(N))
    refs = {i: [[words[w] for w in rng.integers(3, V, size=int(n))] for n in hist_lengths(5, rng, nword)] for i in ids}
    cider = CiderD(refs)
    reward = scst.cider_reward(cider, words)
    dev, t_build = None, None
    if reward_mode != "host":
        from lrcn_amd.cider_device import DeviceCiderD
        t0 = time.perf_counter()
        dev = DeviceCiderD(refs, {w: k for k, w in enumerate(words)}, L.UNK)
        t_build = (time.perf_counter() - t0) * 1e3      # the one-time table build and upload for this corpus
    image_rows = [i for i in ids for _ in range(S)] + ids     # the N S samples' images, then the N greedy captions'
    feats = L.to_jl((rng.standard_normal((N, 4096)) * 0.01).astype(np.float32))
    rows = L.to_jl(feats.repeat_interleave(S, dim=0))
    out = {"N": N, "S": S, "nword": nword, "rows": N * S, "rounds": []}
    for r in range(rounds + 1):     # round 0 warms every shape up and is not reported
        t_s, samples = wall(lambda: L.sample_batch(ctx, param, feats, S, nword, seed=100 + r))
        t_g, greedy = wall(lambda: L.beam_search_batch(ctx, param, feats, 1, nword))
        t_r = t_d = t_hs = diff = None
        tok, n = scst.pack_samples(samples, nword)
        if reward_mode != "device":
            t0 = time.perf_counter()
            tok, n = scst.pack_samples(samples, nword)
            r_s = [[reward(i, scst.sample_words(tok[i, s], n[i, s])) for s in range(S)] for i in ids]
            r_g = [reward(i, scst.sample_words(seq, len(seq))) for i, (seq, _) in zip(ids, greedy)]
            t_hs = (time.perf_counter() - t0) * 1e3     # CiderD.score over all captions plus the Python that feeds it
            tokens, lens, w, nt = scst.build_batch(tok, n, scst.advantages(r_s, r_g))
            t_r = (time.perf_counter() - t0) * 1e3
        if dev is not None:
            # the sampler's arrays as they are, the greedy rows behind them: one score_ids call to the float64 result (copies and the wait inside)
            gt, gn = scst.pack_samples([[g] for g in greedy], nword)
            all_tok = np.concatenate([tok.reshape(N * S, -1), gt.reshape(N, -1)])
            all_len = np.concatenate([n.reshape(-1), gn.reshape(-1)])
            t_d, r_dev = wall(lambda: dev.score_ids(image_rows, all_tok, all_len))
            if reward_mode == "both":
                diff = float(np.abs(r_dev - np.concatenate([np.asarray(r_s, np.float64).reshape(-1), np.asarray(r_g, np.float64)])).max())
            else:
                tokens, lens, w, nt = scst.build_batch(tok, n, scst.advantages(r_dev[:N * S].reshape(N, S), r_dev[N * S:]))
        if not np.count_nonzero(w):
            w[:] = 1.0               # (every reward 0 against random references: time the step all the same)
        t_t, _ = wall(lambda: tr.step(None, tokens, feats=rows, lens=lens, norm_tokens=nt, row_weights=w))
        if r:
            out["rounds"].append({"sample_ms": t_s, "greedy_ms": t_g, "host_reward_ms": t_r, "train_step_ms": t_t, "T": int(tokens.shape[0]),
                                  "mean_words": float(lens.mean()), "zero_weight_share": 1.0 - np.count_nonzero(w) / float(N * S)})
            if t_hs is not None:
                out["rounds"][-1]["host_score_ms"] = t_hs
            if t_d is not None:
                out["rounds"][-1]["device_reward_ms"] = t_d
            if diff is not None:
                out["rounds"][-1]["reward_max_abs_diff"] = diff
    for k in ("sample_ms", "greedy_ms", "host_reward_ms", "host_score_ms", "device_reward_ms", "train_step_ms"):
        if out["rounds"] and out["rounds"][0].get(k) is not None:
            out[k + "_median"] = float(np.median([x[k] for x in out["rounds"]]))
    if dev is not None:
        out["device_table_build_ms"], out["device_stats"] = t_build, dev.stats()
        if reward_mode == "both":
            out["reward_max_abs_diff"] = max(x["reward_max_abs_diff"] for x in out["rounds"])
        dev.close()
    tr.close()
    ctx.close()
    torch.cuda.empty_cache()
    return out


def step_times(B, T, rounds, steps, rng):
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    grads = L.zeros_like_model(param)
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.01).astype(np.float32))
    tok = torch.as_tensor(rng.integers(3, V, size=(T, B)).astype(np.int32)).cuda()
    lens = hist_lengths(B, rng, T)
    lens[0] = T
    nt = int(lens.sum()) + B
    one = np.ones(B, np.float32)
    half = one.copy()
    half[1::2] = 0.0
    seed = [0]

    def run(w):
        def fn():
            seed[0] += 1
            L.train_step(ctx, param, optim, grads, feats, tok, pdrop=0.4, seed=seed[0], lens=lens, norm_tokens=nt, row_weights=w)
        return fn

    fns = {"var": run(None), "w_ones": run(one), "w_half_zero": run(half)}
    for fn in fns.values():
        timed(fn, 10)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, steps))
    ctx.close()
    torch.cuda.empty_cache()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"B": B, "T": T, "mean_len": float(lens.mean()), "ms": ms, "median_ms": med, "var_spread": (max(ms["var"]) - min(ms["var"])) / med["var"],
            "w_ones_over_var": med["w_ones"] / med["var"], "w_half_zero_over_var": med["w_half_zero"] / med["var"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--nword", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reward", default="host", choices=["host", "device", "both"],
                    help="where the split's CIDEr-D runs: host (cider.CiderD), device (cider_device.DeviceCiderD), or both in turn in every round")
    ap.add_argument("--split_only", action="store_true", help="skip the train-step comparison")
    ap.add_argument("--out")
    o = ap.parse_args()
    rng = np.random.default_rng(0)
    sp = step_split(o.images, o.samples, o.nword, o.rounds, rng, o.reward)
    ms = lambda k: "%.2f ms" % sp[k + "_median"] if k + "_median" in sp else "not run"   # noqa: E731
    print("scst step, %d images x %d samples (%d rows), at most %d words, medians of %d rounds: sample %s | greedy %s | host reward %s | "
          "weighted train step %s   (T = %d, %.1f words per sample)"
          % (sp["N"], sp["S"], sp["rows"], sp["nword"], len(sp["rounds"]), ms("sample_ms"), ms("greedy_ms"), ms("host_reward_ms"),
             ms("train_step_ms"), sp["rounds"][-1]["T"], sp["rounds"][-1]["mean_words"]), flush=True)
    if o.reward != "host":
        print("device reward (one score_ids call over the %d samples and %d greedy captions): %s, rounds %s | host scores alone %s, rounds %s | "
              "table build %.1f ms | largest |device - host| %s | %s"
              % (sp["rows"], sp["N"], ms("device_reward_ms"), " ".join("%.3f" % x["device_reward_ms"] for x in sp["rounds"]), ms("host_score_ms"),
                 " ".join("%.3f" % x["host_score_ms"] for x in sp["rounds"] if "host_score_ms" in x), sp["device_table_build_ms"],
                 "%.3g" % sp["reward_max_abs_diff"] if "reward_max_abs_diff" in sp else "not run", sp["device_stats"]), flush=True)
    steps = []
    for B in (() if o.split_only else (256, 32)):
        r = step_times(B, 20, o.rounds, o.steps, rng)
        steps.append(r)
        print("train step B=%3d T=20 (mean length %.1f): lrcn_train_step_var %.3f ms (rounds %s, spread %.2f %%) | lrcn_train_step_w, weights 1: %.3f ms "
              "(rounds %s, ratio %.4f) | every second weight 0: %.3f ms (rounds %s, ratio %.4f)"
              % (B, r["mean_len"], r["median_ms"]["var"], " ".join("%.3f" % v for v in r["ms"]["var"]), 100 * r["var_spread"], r["median_ms"]["w_ones"],
                 " ".join("%.3f" % v for v in r["ms"]["w_ones"]), r["w_ones_over_var"], r["median_ms"]["w_half_zero"],
                 " ".join("%.3f" % v for v in r["ms"]["w_half_zero"]), r["w_half_zero_over_var"]), flush=True)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    summary = {"tool": "scst_bench", "commit": commit, "E": E, "H": H, "V": V, "dtype": "bf16", "split": sp, "step": steps}
    print(json.dumps(summary))
    if o.out:
        with open(o.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
