#!/usr/bin/env python3
"""Constrained beam search (lrcn_beam_constrained_batch, include/lrcn_constrain.h) against the n-best beam (lrcn_beam_nbest_batch) at the same
N and K: time per call and per decode step.  bf16, E = H = 1000, V = 10640, the decisive random model of tools/diverse_bench.py, eos
improbable so that every call runs all nword + 1 steps.  One ban list of --nban words (the words the unconstrained lists use most, so the
list binds), --min_len and --no_repeat_ngram.

Two shapes by default.  512 images x K = 10: the n-best beam is already on the f32-logits route (the fused softmax / top-K epilogue needs
K < 6), so the difference is the constrained kernel against the unconstrained rows kernel.  1024 images x K = 5: the constrained call also
gives up the fused epilogue; the n-best beam under LRCN_DECODE_SMAX=0 is the like-for-like baseline, and both n-best lines are reported.

Every shape is measured in a process of its own, started from here under its own time limit; in it the three calls alternate, each timed on
the host around the synchronous C call.  The first child that fails or runs out of time ends the run.  One JSON line per shape; --md writes
the table as well.  Needs an MI355X.

    python tools/constrained_bench.py [--shapes 512x10 1024x5] [--nban 50] [--min_len 5] [--no_repeat_ngram 3] [--iters 7] [--md profiles/constrained_bench.md]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = H = 1000
V = 10640


def child(o, shape):
    import ctypes as C
    import gc
    import time

    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import lrcn_amd
    from lrcn_amd import _lib
    from lrcn_amd import lrcn as L

    N, K = (int(v) for v in shape.split("x"))
    steps = o.nword + 1
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
    # warm-up (tables, lazily allocated state, pinned staging); the ban list: the words the unconstrained lists use most
    free = L.beam_nbest_batch(ctx, param, fj, K, o.nword, o.alpha)
    count = {}
    for img in free:
        for toks, _, _ in img:
            for t in toks[1:]:
                count[t] = count.get(t, 0) + 1
    ban = sorted((t for t in count if t != lrcn_amd.EOS), key=lambda t: (-count[t], t))[:o.nban]
    ban += [t for t in range(3, V) if t not in count][:o.nban - len(ban)]
    con = L.beam_constrained_batch(ctx, param, fj, K, o.nword, o.alpha, ban, o.min_len, o.no_repeat_ngram)
    for name, imgs in (("nbest", free), ("constrained", con)):
        assert all(len(img) == K and all(len(e[0]) == steps + 1 for e in img) for img in imgs), "%s: an image finished early: per-step times would be off" % name
    changed = sum(1 for a, b in zip(free, con) if [e[0] for e in a] != [e[0] for e in b])
    Lh = o.nword + 2
    tok, ln, v1, v2 = (C.c_int32 * (N * K * Lh))(), (C.c_int * (N * K))(), (C.c_float * (N * K))(), (C.c_float * (N * K))()
    p9, fp = L._p9(param), L._ptr(fj)
    arr = (C.c_int32 * len(ban))(*ban)
    cons = _lib.Constraints(arr, len(ban), o.min_len, o.no_repeat_ngram)

    def rows_route():   # the n-best beam with the fused softmax / top-K epilogue switched off: the constrained call's own route
        os.environ["LRCN_DECODE_SMAX"] = "0"
        try:
            ctx._call("lrcn_beam_nbest_batch", p9, fp, N, K, o.nword, float(o.alpha), tok, ln, v1, v2)
        finally:
            del os.environ["LRCN_DECODE_SMAX"]

    fns = {"nbest": lambda: ctx._call("lrcn_beam_nbest_batch", p9, fp, N, K, o.nword, float(o.alpha), tok, ln, v1, v2),
           "nbest_rows": rows_route,
           "constrained": lambda: ctx._call("lrcn_beam_constrained_batch", p9, fp, N, K, 0, 0.0, o.nword, float(o.alpha), C.byref(cons), tok, ln, v1, v2)}
    gc.collect()
    gc.freeze()   # (tools/beam_bench.py: keep full cyclic-GC passes out of the timed decodes)
    times = {k: [] for k in fns}
    for _ in range(o.iters):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()   # returns after its results are on the host
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"images": N, "K": K, "nban": len(ban), "min_len": o.min_len, "no_repeat_ngram": o.no_repeat_ngram, "nword": o.nword, "steps": steps,
           "alpha": o.alpha, "iters": o.iters, "images_changed": changed}
    for k in fns:
        t = np.array(times[k])
        out[k] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                  "ms_per_step": round(float(np.median(t)) / steps, 4)}
    out["constrained_over_nbest"] = round(out["constrained"]["ms_median"] / out["nbest"]["ms_median"], 4)
    out["constrained_over_nbest_rows"] = round(out["constrained"]["ms_median"] / out["nbest_rows"]["ms_median"], 4)
    print(json.dumps(out))
    ctx.close()
    return 0


def table(rows):
    r0 = rows[0]
    lines = ["# Constrained beam search against the n-best beam (tools/constrained_bench.py)", "",
             "bf16, E = H = 1000, V = 10640, nword %d (%d decode steps, eos improbable: no early stop), alpha %g; %d banned words (the words the "
             "unconstrained lists use most), min_len %d, no_repeat_ngram %d; median of %d calls each, the three calls alternating in one process "
             "per shape, host time around the synchronous call.  `n-best` is lrcn_beam_nbest_batch on the route its router picks, `n-best, f32 "
             "logits` the same call under LRCN_DECODE_SMAX=0 (the constrained call's own route: the like-for-like baseline; at K = 10 the two are "
             "the same route)." %
             (r0["nword"], r0["steps"], r0["alpha"], r0["nban"], r0["min_len"], r0["no_repeat_ngram"], r0["iters"]), "",
             "| images | K | rows | n-best ms | n-best, f32 logits ms | constrained ms (min .. max) | constrained / n-best | constrained / n-best, f32 logits | "
             "ms per step: n-best | n-best, f32 logits | constrained | images whose list changed |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a, b, c = r["nbest"], r["nbest_rows"], r["constrained"]
        lines.append("| %d | %d | %d | %.3f | %.3f | %.3f (%.3f .. %.3f) | %.4f | %.4f | %.4f | %.4f | %.4f | %d |" %
                     (r["images"], r["K"], r["images"] * r["K"], a["ms_median"], b["ms_median"], c["ms_median"], c["ms_min"], c["ms_max"],
                      r["constrained_over_nbest"], r["constrained_over_nbest_rows"], a["ms_per_step"], b["ms_per_step"], c["ms_per_step"],
                      r["images_changed"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["512x10", "1024x5"], help="images x beam width")
    ap.add_argument("--nban", type=int, default=50)
    ap.add_argument("--min_len", type=int, default=5)
    ap.add_argument("--no_repeat_ngram", type=int, default=3)
    ap.add_argument("--nword", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--limit", type=int, default=150, help="seconds each shape's process may take")
    ap.add_argument("--md", default="", help="write the table here as well")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    o = ap.parse_args()
    if o.child:
        return child(o, o.child)
    rows = []
    for shape in o.shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape] + [a for a in sys.argv[1:]]
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=o.limit)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (shape, o.limit), file=sys.stderr)
            return 1
        if res.returncode != 0:
            print("%s: exit status %d; stopping" % (shape, res.returncode), file=sys.stderr)
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
