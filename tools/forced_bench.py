#!/usr/bin/env python3
"""Forced-word beam search (lrcn_beam_forced_batch, include/lrcn_forced.h) against the constrained n-best beam it is built on
(lrcn_beam_constrained_batch on the f32-logits route, with a constraint that cannot bind: no_repeat_ngram = nword + 2): time per call and
per decode step.  bf16, E = H = 1000, V = 10640, the decisive random model of tools/constrained_bench.py, eos improbable so that every call
runs all nword + 1 steps.  A forced call with C sets at width K decodes S * K rows per image, S = 2^C; it is compared with the constrained
beam at width S * K (the same rows) and at width K (the same output).  The sets hold words that the unforced lists do not use, so they bind
on every image.

Every shape is measured in a process of its own, started from here under its own time limit; in it the three calls alternate, each timed on
the host around the synchronous C call.  The first child that fails or runs out of time ends the run.  One JSON line per shape; --md writes
the table as well.  Needs an MI355X.

    python tools/forced_bench.py [--shapes 1x5 2x5] [--images 256] [--alts 2] [--iters 7] [--md profiles/forced_bench.md]
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

    Cn, K = (int(v) for v in shape.split("x"))
    N, S, steps = o.images, 1 << Cn, o.nword + 1
    W = S * K
    ctx = L.Context(E, H, H, V, max_B=N * W, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16)
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
    ngram = o.nword + 2   # cannot bind: the f32-logits route with the constrained kernel, nothing else
    # warm-up (tables, lazily allocated state, pinned staging); the sets: words the unforced lists at the wide width do not use
    wide = L.beam_constrained_batch(ctx, param, fj, W, o.nword, o.alpha, (), 0, ngram)
    narrow = L.beam_constrained_batch(ctx, param, fj, K, o.nword, o.alpha, (), 0, ngram)
    used = set(t for img in wide for toks, _, _ in img for t in toks)
    free = [t for t in range(3, V) if t not in used]
    sets = [free[c * o.alts:(c + 1) * o.alts] for c in range(Cn)]
    forced = L.beam_forced_batch(ctx, param, fj, K, o.nword, o.alpha, sets, (), 0, ngram)
    for name, imgs, width in (("wide", wide, W), ("narrow", narrow, K), ("forced", forced, K)):
        assert all(len(img) == width and all(len(e[0]) == steps + 1 for e in img) for img in imgs), "%s: an image finished early or is short of entries" % name
    assert all(L.meets(toks, sets) for img in forced for toks, _, _ in img)
    Lh = o.nword + 2
    tok, ln, v1, v2 = (C.c_int32 * (N * W * Lh))(), (C.c_int * (N * W))(), (C.c_float * (N * W))(), (C.c_float * (N * W))()
    p9, fp = L._p9(param), L._ptr(fj)
    cons = _lib.Constraints(None, 0, 0, ngram)
    fw, keep, _ = L._forced(sets, N)

    def constrained(width):
        return lambda: ctx._call("lrcn_beam_constrained_batch", p9, fp, N, width, 0, 0.0, o.nword, float(o.alpha), C.byref(cons), tok, ln, v1, v2)

    fns = {"constrained_rows": constrained(W), "constrained_K": constrained(K),
           "forced": lambda: ctx._call("lrcn_beam_forced_batch", p9, fp, N, K, o.nword, float(o.alpha), C.byref(cons), C.byref(fw), tok, ln, v1, v2)}
    gc.collect()
    gc.freeze()   # (tools/beam_bench.py: keep full cyclic-GC passes out of the timed decodes)
    times = {k: [] for k in fns}
    for _ in range(o.iters):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()   # returns after its results are on the host
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"images": N, "C": Cn, "A": o.alts, "K": K, "rows": N * W, "nword": o.nword, "steps": steps, "alpha": o.alpha, "iters": o.iters}
    for k in fns:
        t = np.array(times[k])
        out[k] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                  "ms_per_step": round(float(np.median(t)) / steps, 4)}
    out["forced_over_rows"] = round(out["forced"]["ms_median"] / out["constrained_rows"]["ms_median"], 4)
    out["forced_over_K"] = round(out["forced"]["ms_median"] / out["constrained_K"]["ms_median"], 4)
    print(json.dumps(out))
    del keep
    ctx.close()
    return 0


def table(rows):
    r0 = rows[0]
    lines = ["# Forced-word beam search against the constrained n-best beam (tools/forced_bench.py)", "",
             "bf16, E = H = 1000, V = 10640, %d images, nword %d (%d decode steps, eos improbable: no early stop), alpha %g; C sets of %d "
             "alternatives, words that the unforced lists do not use; every call carries no_repeat_ngram = nword + 2, which cannot bind and puts "
             "the constrained beam on the f32-logits route the forced call runs on.  Median of %d calls each, the three calls alternating in one "
             "process per shape, host time around the synchronous call.  `same rows` is lrcn_beam_constrained_batch at width 2^C * K, `same "
             "output` at width K." % (r0["images"], r0["nword"], r0["steps"], r0["alpha"], r0["A"], r0["iters"]), "",
             "| C | K | rows | constrained, same rows ms (min .. max) | constrained, same output ms (min .. max) | forced ms (min .. max) | "
             "forced / same rows | forced / same output | ms per step: same rows | same output | forced |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        a, b, c = r["constrained_rows"], r["constrained_K"], r["forced"]
        lines.append("| %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.4f | %.4f | %.4f | %.4f | %.4f |" %
                     (r["C"], r["K"], r["rows"], a["ms_median"], a["ms_min"], a["ms_max"], b["ms_median"], b["ms_min"], b["ms_max"],
                      c["ms_median"], c["ms_min"], c["ms_max"], r["forced_over_rows"], r["forced_over_K"], a["ms_per_step"], b["ms_per_step"],
                      c["ms_per_step"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["1x5", "2x5"], help="sets x beam width")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--alts", type=int, default=2, help="alternatives per set")
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
