"""Variable-length caption batches (include/lrcn_varlen.h) on one GPU at the benchmark's caption shape (E = H = 1000, V = 10640, bf16):

  step   lrcn_train_step_var with every length = T against lrcn_train_step at the same B and T, alternated in one process: the masked path
         launches the same chain, so it should cost what the existing path costs; the margin is the spread of this run's own equal-length
         rounds.
  eval   train.average_loss over one synthetic validation split of 25 000 captions (lengths from the COCO reference captions' histogram)
         two ways: the reference's batcher (forced batch 10, equal lengths) and the padded batches at 256 rows.  Both times, both losses.

Prints one line per measurement and a JSON summary line.
usage: python tools/varlen_bench.py [--rounds 5] [--steps 30] [--captions 25000] [--rows 256] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lrcn_amd
from lrcn_amd import captions as cap
from lrcn_amd import dp
from lrcn_amd import lrcn as L
from lrcn_amd import train as trn

E = H = 1000
V = 10640
# word counts of the 5000 COCO reference captions of the evaluation set: the fixture the host tests check the batcher on
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "coco_ref_caption_lengths.json")) as _fh:
    HIST = {int(k): v for k, v in json.load(_fh)["histogram"].items()}


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def step_times(B, T, rounds, steps, rng):
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    grads = L.zeros_like_model(param)
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.01).astype(np.float32))
    tok = torch.as_tensor(rng.integers(3, V, size=(T, B)).astype(np.int32)).cuda()
    lens = np.full(B, T, np.int32)
    seed = [0]

    def equal():
        seed[0] += 1
        L.train_step(ctx, param, optim, grads, feats, tok, pdrop=0.4, seed=seed[0])

    def masked():
        seed[0] += 1
        L.train_step(ctx, param, optim, grads, feats, tok, pdrop=0.4, seed=seed[0], lens=lens, norm_tokens=B * (T + 1))

    for fn in (equal, masked):
        timed(fn, 10)
    eq, mk = [], []
    for _ in range(rounds):
        eq.append(timed(equal, steps) * 1e3)
        mk.append(timed(masked, steps) * 1e3)
    ctx.close()
    torch.cuda.empty_cache()
    return eq, mk


def synthetic_split(n, rng):
    """n captions with HIST's lengths (scaled), random word ids, 5 per image -> (caps sorted by length, vocabulary)."""
    lens = np.repeat(list(HIST), [v * n // 5000 for v in HIST.values()])
    lens.sort(kind="stable")
    vocab = {cap.EOS_WORD: cap.EOS, cap.BOS_WORD: cap.BOS, cap.UNK_WORD: cap.UNK}
    for k in range(V - 3):
        vocab["w%d" % k] = k + 4
    caps = [((i // 5, ["w%d" % w for w in rng.integers(0, V - 3, size=int(ln))]), int(ln)) for i, ln in enumerate(lens)]
    return caps, vocab


def eval_times(n_caps, rows, rng):
    caps, vocab = synthetic_split(n_caps, rng)
    ctx = L.Context(E, H, H, V, max_B=max(rows, 10), lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    table = torch.as_tensor((rng.standard_normal((n_caps // 5 + 1, 4096)) * 0.01).astype(np.float32)).cuda()

    def feats_of(ids):
        return L.to_jl(table[torch.as_tensor(ids, device=table.device)])

    tr = types.SimpleNamespace(world=1, rank=0, ops=dp.HipOps(ctx), param=param, group=None)
    seq = cap.minibatch(caps, vocab, rows)                       # <= 30000 captions: forced to batch 10 (lrcn.jl:260-270)
    ref_blocks = list(cap.batches(seq[0], seq[1], seq[2], seq[3]))
    var_blocks = cap.minibatch_varlen(caps, vocab, rows)
    out = {"captions": len(caps), "rows": rows}
    for name, blocks in (("reference_batch10", ref_blocks), ("varlen", list(var_blocks))):
        trn.average_loss(tr, blocks[:20], feats_of)              # warm-up: lazily allocated scratch, first-launch costs
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val = trn.average_loss(tr, blocks, feats_of)
        torch.cuda.synchronize()
        out[name] = {"seconds": time.perf_counter() - t0, "loss": val, "batches": len(blocks), "captions_scored": sum(len(b[0]) for b in blocks)}
    out["varlen"]["padded_share"] = var_blocks.padded_share
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--captions", type=int, default=25000)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--out")
    o = ap.parse_args()
    rng = np.random.default_rng(0)
    steps = []
    for B in (256, 32):
        eq, mk = step_times(B, 11, o.rounds, o.steps, rng)
        r = {"B": B, "T": 11, "equal_ms": eq, "masked_ms": mk, "equal_median_ms": float(np.median(eq)), "masked_median_ms": float(np.median(mk)),
             "equal_spread": (max(eq) - min(eq)) / float(np.median(eq))}
        r["masked_over_equal"] = r["masked_median_ms"] / r["equal_median_ms"]
        steps.append(r)
        print("step B=%3d T=11: lrcn_train_step %.3f ms (rounds %s)  lrcn_train_step_var %.3f ms (rounds %s)  ratio %.4f, equal-length spread %.2f %%"
              % (B, r["equal_median_ms"], " ".join("%.3f" % v for v in eq), r["masked_median_ms"], " ".join("%.3f" % v for v in mk),
                 r["masked_over_equal"], 100 * r["equal_spread"]), flush=True)
    ev = eval_times(o.captions, o.rows, rng)
    a, b = ev["reference_batch10"], ev["varlen"]
    print("average_loss over %d captions: reference batcher (batch 10) %.2f s, %d batches, %d captions scored, loss %.5f | padded batches of %d: "
          "%.2f s, %d batches, %d captions scored, loss %.5f, %.1f %% of the rows are padding -> %.1fx"
          % (ev["captions"], a["seconds"], a["batches"], a["captions_scored"], a["loss"], ev["rows"], b["seconds"], b["batches"],
             b["captions_scored"], b["loss"], 100 * b["padded_share"], a["seconds"] / b["seconds"]), flush=True)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    summary = {"tool": "varlen_bench", "commit": commit, "E": E, "H": H, "V": V, "dtype": "bf16", "step": steps, "eval": ev}
    print(json.dumps(summary))
    if o.out:
        with open(o.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
