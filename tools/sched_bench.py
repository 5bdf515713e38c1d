"""What scheduled sampling (include/lrcn_sched.h) costs per training step on one GPU, at the benchmark's caption shape (E = H = 1000,
V = 10640, T = 20, bf16): ms per lrcn_train_step_sched at eps 0, 0.25 and 1 against lrcn_train_step_var on the same batch, at 256 and 32
rows, all in one process and alternated round by round.  eps 0 takes the time-batched route (it must cost what lrcn_train_step_var costs,
within the spread of that call's own two columns); eps > 0 runs the forward step by step, about nine launches per step in place of one
time-batched chain.

Every variant of a shape is warmed up before the first timed round; a round times `steps` calls between two device synchronisations; the
table reports medians over the rounds and the rounds' spread.  lrcn_train_step_var is timed TWICE per round (first and last), so the table
shows what two runs of the same call differ by.

usage: python tools/sched_bench.py [--rounds 7] [--steps 30] [--out profiles/sched_bench.md]"""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import lrcn_amd
from lrcn_amd import lrcn as L

E = H = 1000
V = 10640
T = 20
EPS = (0.0, 0.25, 1.0)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def step_times(B, rounds, steps, rng):
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    grads = L.zeros_like_model(param)
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.01).astype(np.float32))
    tok = torch.as_tensor(rng.integers(3, V, size=(T, B)).astype(np.int32)).cuda()
    lens = np.full(B, T, np.int32)
    seed = [0]

    def var():
        seed[0] += 1
        L.train_step(ctx, param, optim, grads, feats, tok, pdrop=0.4, seed=seed[0], lens=lens, norm_tokens=B * (T + 1))

    def sched(eps):
        def f():
            seed[0] += 1
            L.train_step(ctx, param, optim, grads, feats, tok, pdrop=0.4, seed=seed[0], lens=lens, norm_tokens=B * (T + 1),
                         sched=(eps, 1.0, seed[0]))
        return f

    variants = [("var", var)] + [("eps%g" % e, sched(e)) for e in EPS] + [("var_again", var)]
    for _, fn in variants:
        timed(fn, 10)
    ms = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            ms[name].append(timed(fn, steps) * 1e3)
    rate = {}
    for e in EPS[1:]:   # the realised draw rate of one more call each
        sched(e)()
        el, dr = L.sched_stats(ctx)
        rate["eps%g" % e] = dr / max(el, 1)
    ctx.close()
    torch.cuda.empty_cache()
    return ms, rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out")
    o = ap.parse_args()
    rng = np.random.default_rng(0)
    rows, results = [], []
    for B in (256, 32):
        ms, rate = step_times(B, o.rounds, o.steps, rng)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
        results.append({"B": B, "T": T, "ms": ms, "median_ms": med, "spread": spread, "drawn_over_eligible": rate})
        for k in ("var", "var_again", "eps0", "eps0.25", "eps1"):
            rows.append("| %d | %s | %.3f | %.3f | %.3f | %.1f %% |" % (B, {"var": "`lrcn_train_step_var`", "var_again": "`lrcn_train_step_var` (again)",
                                                                         "eps0": "sched, eps 0", "eps0.25": "sched, eps 0.25", "eps1": "sched, eps 1"}[k],
                                                                     med[k], min(ms[k]), med[k] / med["var"], 100 * spread[k]))
            print(rows[-1], flush=True)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    summary = {"tool": "sched_bench", "commit": commit, "E": E, "H": H, "V": V, "T": T, "dtype": "bf16", "rounds": o.rounds, "steps": o.steps,
               "device": torch.cuda.get_device_name(0), "step": results}
    print(json.dumps(summary))
    if o.out:
        with open(o.out, "w") as fh:
            fh.write("# Scheduled sampling: ms per training step (tools/sched_bench.py)\n\n")
            fh.write("%s, E = H = %d, V = %d, T = %d, bf16, dropout 0.4, every length = T; %d rounds of %d steps per variant, alternated in one "
                     "process after a warm-up of every variant; median over the rounds, `spread` = (max - min) / median of the rounds.  "
                     "`lrcn_train_step_var` is timed first and last in every round: the two rows show what two runs of one call differ by.\n\n"
                     % (summary["device"], E, V, T, o.rounds, o.steps))
            fh.write("| rows | call | median ms | best ms | / `lrcn_train_step_var` | spread |\n|---|---|---|---|---|---|\n")
            fh.write("\n".join(rows) + "\n\n")
            fh.write("Realised drawn / eligible of one call: " + "; ".join("%d rows %s" % (r["B"], ", ".join("%s: %.3f" % kv for kv in r["drawn_over_eligible"].items()))
                                                                          for r in results) + ".\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
