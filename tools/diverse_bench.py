#!/usr/bin/env python3
"""Diverse beam search (lrcn_beam_diverse_batch) against the n-best beam (lrcn_beam_nbest_batch) at the same N and K: time per call and
per decode step, and how diverse the two lists are (distinct-1 / distinct-2 and the mean pairwise unigram overlap of an image's K captions,
averaged over the images; lrcn_amd/diversity.py).  bf16, E = H = 1000, V = 10640, a decisive random model as tools/nbest_bench.py makes it,
eos improbable so that every call runs all nword + 1 steps and call time / (nword + 1) is the cost of one decode step with its
bookkeeping kernel.

Every group count is measured in a process of its own, started from here under its own time limit; in it the two entry points alternate,
each call timed on the host around the synchronous C call.  The first child that fails or runs out of time ends the run.  One JSON line per
group count; --md writes the table as well.  Needs an MI355X.

    python tools/diverse_bench.py [--images 512] [--beam 10] [--groups 1 2 5 10] [--strength 0.5] [--iters 7] [--md profiles/diverse_bench.md]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = H = 1000
V = 10640


def child(o, G):
    import ctypes as C
    import gc
    import time

    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import lrcn_amd
    from lrcn_amd import diversity
    from lrcn_amd import lrcn as L

    N, K, steps = o.images, o.beam, o.nword + 1
    ctx = L.Context(E, H, H, V, max_B=N * K, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=4)
    ctx.sync()
    torch.manual_seed(4)
    with torch.no_grad():   # decisive: W1, W2 x 2, Wout x 16, bout ~ N(0, 2), b1 + N(0, 0.5); eos improbable
        param[0].mul_(2.0)
        param[2].mul_(2.0)
        param[7].mul_(16.0)
        param[8].copy_(torch.randn_like(param[8]) * 2.0)
        param[1].add_(torch.randn_like(param[1]) * 0.5)
        param[8][0, lrcn_amd.EOS] = -30.0
    torch.cuda.synchronize()
    fj = L.to_jl((np.random.default_rng(11).standard_normal((N, 4096)) * 0.05).astype(np.float32))
    # warm-up (tables, lazily allocated state, pinned staging) and the lists whose diversity is reported
    lists = {"nbest": [[e[0][1:] for e in img] for img in L.beam_nbest_batch(ctx, param, fj, K, o.nword, o.alpha)],
             "diverse": [[e[0][1:] for grp in img for e in grp] for img in L.beam_diverse_batch(ctx, param, fj, K, G, o.strength, o.nword, o.alpha)]}
    for name, imgs in lists.items():
        assert all(len(img) == K and all(len(t) == steps for t in img) for img in imgs), "%s: an image finished early: per-step times would be off" % name
    Lh = o.nword + 2
    tok, ln, v1, v2 = (C.c_int32 * (N * K * Lh))(), (C.c_int * (N * K))(), (C.c_float * (N * K))(), (C.c_float * (N * K))()
    p9, fp = L._p9(param), L._ptr(fj)
    fns = {"nbest": lambda: ctx._call("lrcn_beam_nbest_batch", p9, fp, N, K, o.nword, float(o.alpha), tok, ln, v1, v2),
           "diverse": lambda: ctx._call("lrcn_beam_diverse_batch", p9, fp, N, K, G, float(o.strength), o.nword, float(o.alpha), tok, ln, v1, v2)}
    gc.collect()
    gc.freeze()   # (tools/beam_bench.py: keep full cyclic-GC passes out of the timed decodes)
    times = {k: [] for k in fns}
    for _ in range(o.iters):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()   # returns after its results are on the host
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"images": N, "K": K, "G": G, "strength": o.strength, "nword": o.nword, "steps": steps, "alpha": o.alpha, "iters": o.iters}
    for k in fns:
        t = np.array(times[k])
        imgs = lists[k]
        out[k] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                  "ms_per_step": round(float(np.median(t)) / steps, 4),
                  "distinct_1": round(float(np.mean([diversity.distinct_n(img, 1) for img in imgs])), 4),
                  "distinct_2": round(float(np.mean([diversity.distinct_n(img, 2) for img in imgs])), 4),
                  "overlap_1": round(float(np.mean([diversity.mean_pairwise_overlap(img) for img in imgs])), 4)}
    out["diverse_over_nbest"] = round(float(np.median(times["diverse"])) / float(np.median(times["nbest"])), 4)
    print(json.dumps(out))
    ctx.close()
    return 0


def table(rows):
    r0 = rows[0]
    lines = ["# Diverse beam search against the n-best beam (tools/diverse_bench.py)", "",
             "%d images x K = %d (%d rows), nword %d (%d decode steps, eos improbable: no early stop), bf16, E = H = 1000, V = 10640, strength %g, "
             "alpha %g; median of %d calls each, the two entry points alternating in one process per group count, host time around the synchronous "
             "call.  distinct-n and the pairwise unigram overlap are per image over its K captions, averaged over the images; the model is random "
             "and its captions repeat a few words at every position, which is why distinct-1 is low in both lists." %
             (r0["images"], r0["K"], r0["images"] * r0["K"], r0["nword"], r0["steps"], r0["strength"], r0["alpha"], r0["iters"]), "",
             "| G | K' | n-best ms | diverse ms (min .. max) | diverse / n-best | ms per step, n-best | ms per step, diverse | distinct-1 n-best | distinct-1 diverse | "
             "distinct-2 n-best | distinct-2 diverse | overlap n-best | overlap diverse |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a, d = r["nbest"], r["diverse"]
        lines.append("| %d | %d | %.3f | %.3f (%.3f .. %.3f) | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f |" %
                     (r["G"], r["K"] // r["G"], a["ms_median"], d["ms_median"], d["ms_min"], d["ms_max"], r["diverse_over_nbest"], a["ms_per_step"],
                      d["ms_per_step"], a["distinct_1"], d["distinct_1"], a["distinct_2"], d["distinct_2"], a["overlap_1"], d["overlap_1"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--beam", type=int, default=10)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 5, 10])
    ap.add_argument("--strength", type=float, default=0.5)
    ap.add_argument("--nword", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds each group count's process may take")
    ap.add_argument("--md", default="", help="write the table here as well")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    o = ap.parse_args()
    if o.child:
        return child(o, o.child)
    rows = []
    for G in o.groups:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(G)] + [a for a in sys.argv[1:]]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=o.limit)
        except subprocess.TimeoutExpired:
            print("G = %d: no result within %d s; stopping" % (G, o.limit), file=sys.stderr)
            return 1
        if res.returncode != 0:
            print("G = %d: exit status %d; stopping" % (G, res.returncode), file=sys.stderr)
            return 1
        line = res.stdout.decode().strip().splitlines()[-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    if o.md:
        with open(o.md, "w") as fh:
            fh.write(table(rows))
    return 0


if __name__ == "__main__":
    sys.exit(main())
