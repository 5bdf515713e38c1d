"""What label smoothing (include/lrcn_smooth.h) costs on one GPU, at the two caption shapes of the benchmark in bf16:

  C4  12 steps x 256 rows, V = 10640      C3  13 steps x 128 rows, V = 7730      (E = H = 1000, two layers)

  xent   the cross-entropy stage alone (lrcn_xent_logits on random logits N(0, 3^2), bf16 d(logits), every row active), eps = 0 -- the
         masked kernel of lrcn_loss_grad_var -- against eps = 0.1, the SMOOTH form of the same rung
  step   the caption training step on precomputed features (lrcn_train_step_var against lrcn_train_step_smooth), pdrop 0.4

Both settings run in ONE process and alternate round by round, after a warm-up of each; a round is `--iters` launches (xent) or `--steps`
steps between two device synchronisations, timed on the host clock.  Per setting: the median over the rounds and their spread (min .. max);
the ratio is of the medians.  The shader clock the device held is sampled over the whole timed part (bench.HwSampler).  There is no
pass / fail: eps = 0 runs the kernels it ran before the option existed, and the eps > 0 ratio is a number to record.

--row-weights: every call also carries per-caption weights, all 1.0 -- the WEIGHTED form of the loss kernels against its SMOOTH form.

Writes profiles/smooth_bench.md (with --row-weights: profiles/smooth_bench_weighted.md; --out names another file) and prints a JSON
summary line.
usage: python tools/smooth_bench.py [--rounds 7] [--iters 200] [--steps 30] [--row-weights] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import lrcn_amd
from lrcn_amd import lrcn as L

E = H = 1000
SHAPES = {"C4": (11, 256, 10640), "C3": (12, 128, 7730)}   # name -> (T, rows, V)
EPS = (0.0, 0.1)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6   # us per call


def alternate(fns, rounds, n, warm):
    """fns: {eps: callable}.  -> {eps: [us per call of every round]}, the settings taking turns."""
    for fn in fns.values():
        timed(fn, warm)
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(timed(fn, n))
    return out


def summary(us):
    a = np.sort(np.asarray(us))
    return {"median_us": float(np.median(a)), "min_us": float(a[0]), "max_us": float(a[-1]), "rounds": len(a)}


def bench_shape(name, rounds, iters, steps, row_weights):
    T, B, V = SHAPES[name]
    M = (T + 1) * B
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_BF16)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    ld = (V + 63) // 64 * 64   # the context's own leading dimension of its logits
    logits = (torch.randn((M, ld), generator=g, device="cuda") * 3.0)[:, :V]
    rng = np.random.default_rng(1)
    tgt = torch.as_tensor(rng.integers(0, V, size=M).astype(np.int32)).cuda()
    w = torch.ones(B, device="cuda") if row_weights else None
    xent = {eps: (lambda eps=eps: L.xent_logits(ctx, logits, tgt, row_weights=w, B=B, scale=1.0 / M, label_smoothing=eps, out_dtype=torch.bfloat16,
                                                ld_d=ld))
            for eps in EPS}
    res = {"xent": {str(k): summary(v) for k, v in alternate(xent, rounds, iters, 20).items()}}
    param = L.initweights(ctx, seed=42)
    optim = L.initparams(param)
    grads = [L.jl_empty(*t.shape) for t in param]
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.02).astype(np.float32))
    toks = torch.as_tensor(rng.integers(3, V, size=(T, B)).astype(np.int32)).cuda()
    lens = np.full(B, T, np.int32)
    wh = np.ones(B, np.float32) if row_weights else None
    step = {eps: (lambda eps=eps: L.train_step(ctx, param, optim, grads, feats, toks, pdrop=0.4, seed=optim.t, lens=lens, row_weights=wh,
                                               label_smoothing=eps))
            for eps in EPS}
    res["step"] = {str(k): summary(v) for k, v in alternate(step, rounds, steps, 10).items()}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--row-weights", action="store_true", help="per-caption weights of 1.0 in every call: the weighted forms")
    ap.add_argument("--out", default=None, help="default profiles/smooth_bench.md, with --row-weights profiles/smooth_bench_weighted.md")
    a = ap.parse_args()
    from bench import HwSampler
    hw = HwSampler(torch.cuda.current_device())
    hw.start()
    res = {name: bench_shape(name, a.rounds, a.iters, a.steps, a.row_weights) for name in SHAPES}
    clock = hw.stop()
    sclk = (clock.get("sclk_mhz") or {}) if clock.get("available") else {}
    a.out = a.out or os.path.join(ROOT, "profiles", "smooth_bench_weighted.md" if a.row_weights else "smooth_bench.md")
    lines = ["# Label smoothing: the cost of the SMOOTH loss kernels" + (", with per-caption weights" if a.row_weights else ""), "",
             "`python tools/smooth_bench.py --rounds %d --iters %d --steps %d%s` on %s; bf16, E = H = 1000, two layers.  eps = 0 and eps = 0.1"
             % (a.rounds, a.iters, a.steps, " --row-weights" if a.row_weights else "", torch.cuda.get_device_name()),
             "alternate round by round in one process after a warm-up of each; a round is that many launches (xent) or steps between two device",
             "synchronisations on the host clock.  Median over the rounds, spread = min .. max.  Shader clock over the timed part: %s."
             % ("median %.0f MHz (min %.0f, max %.0f)" % (sclk["median"], sclk.get("min", float("nan")), sclk.get("max", float("nan")))
                if sclk.get("median") is not None else "not available"), "",
             "| shape | what | eps = 0 (us) | spread | eps = 0.1 (us) | spread | ratio of medians |", "|---|---|---|---|---|---|---|"]
    for name, r in res.items():
        T, B, V = SHAPES[name]
        for what, label in (("xent", "xent stage alone, %d x %d rows, V = %d" % (T + 1, B, V)), ("step", "training step (LSTM side)")):
            z, s = r[what]["0.0"], r[what]["0.1"]
            lines.append("| %s | %s | %.1f | %.1f .. %.1f | %.1f | %.1f .. %.1f | %.3f |"
                         % (name, label, z["median_us"], z["min_us"], z["max_us"], s["median_us"], s["min_us"], s["max_us"], s["median_us"] / z["median_us"]))
    lines += ["", "The xent rows include the launch of the target check of lrcn_xent_logits (one small kernel) in both settings.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    print(json.dumps({"smooth_bench": res, "sclk_mhz": sclk}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
