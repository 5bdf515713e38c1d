#!/usr/bin/env python3
"""n-best beam search (lrcn_beam_nbest_batch) against the reference beam (lrcn_beam_search_batch) at the production decode shape:
1024 images x K = 5, nword 30, bf16, E = H = 1000, V = 10640, on a decisive random model (initweights scaled as in
tests/test_gpu_decode_epilogue.py).  eos is made improbable (its output bias at -30), so no image of either entry point finishes early:
both run all nword + 1 decode steps, and call time / (nword + 1) is the cost of one decode step including each one's per-step choice
kernels.  The two C entry points alternate in one process, writing into preallocated host arrays; every call is synchronised and timed
with events.  One JSON line: per entry point
the median / min / max call time, captions/s and ms per decode step, and the n-best / beam ratio of ms per step.  Needs an MI355X.

    python tools/nbest_bench.py [--iters 10] [--alpha 0]
"""
import argparse
import ctypes as C
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lrcn_amd  # noqa: E402
from lrcn_amd import lrcn as L  # noqa: E402

E = H = 1000
V = 10640


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--nword", type=int, default=30)
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=10)
    o = ap.parse_args()
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
    first = {"beam": L.beam_search_batch(ctx, param, fj, K, o.nword),   # warm-up: tables, lazily allocated state, pinned staging
             "nbest": L.beam_nbest_batch(ctx, param, fj, K, o.nword, o.alpha)}
    assert all(len(t) == o.nword + 2 for t, _ in first["beam"]), "an image finished early: per-step times would be off"
    assert all(len(e[0]) == o.nword + 2 for img in first["nbest"] for e in img), "an image finished early: per-step times would be off"
    # the timed calls: the C entry points themselves into preallocated host arrays (no Python-side conversion of the results)
    Lh = o.nword + 2
    tok, ln, v1, v2 = (C.c_int32 * (N * K * Lh))(), (C.c_int * (N * K))(), (C.c_float * (N * K))(), (C.c_float * (N * K))()
    p9, fp = L._p9(param), L._ptr(fj)
    fns = {"beam": lambda: ctx._call("lrcn_beam_search_batch", p9, fp, N, K, o.nword, tok, ln, v1),
           "nbest": lambda: ctx._call("lrcn_beam_nbest_batch", p9, fp, N, K, o.nword, float(o.alpha), tok, ln, v1, v2)}
    gc.collect()
    gc.freeze()   # (tools/beam_bench.py: keep full cyclic-GC passes out of the timed decodes)
    times = {k: [] for k in fns}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(o.iters):
        for k, f in fns.items():
            torch.cuda.synchronize()
            ev0.record()
            f()
            ev1.record()
            ev1.synchronize()
            times[k].append(ev0.elapsed_time(ev1))
    out = {"images": N, "K": K, "nword": o.nword, "steps": steps, "alpha": o.alpha, "iters": o.iters}
    for k in fns:
        t = np.array(times[k])
        out[k] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                  "captions_per_s": round(N / (float(np.median(t)) / 1e3), 1), "ms_per_step": round(float(np.median(t)) / steps, 4)}
    out["nbest_over_beam_per_step"] = round(float(np.median(times["nbest"])) / float(np.median(times["beam"])), 4)
    print(json.dumps(out))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
