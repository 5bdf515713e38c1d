#!/usr/bin/env python3
"""Sampled caption generation throughput (lrcn_sample_batch, lrcn_sample_batch_p) at the C5 decode shape, 1 GPU: E = H = 1000, V = 10640,
1024 images x S = 5 samples = 5120 rows, nword = 30, bf16, random weights (initweights) and features.  One line per route of the per-step
draw -- the Gumbel records of the logits GEMM (top_k 0), the top-K records (top_k 3), the row kernel on plain logits (LRCN_DECODE_SMAX=0;
top_k 0 and 10) -- and beam search of width 5 over the same 5120 rows for comparison.  rows/s = rows x steps run / s; captions/s = N x S / s.
--topp P and / or --topk K (include/lrcn_nucleus.h) add one line for that nucleus / wide top_k configuration, which runs on the plain-logits
route: compare it with the "row kernel, top_k 0 (LRCN_DECODE_SMAX=0)" line.  --nword sets the caption length, --only-nucleus skips the rest.
Kernel times per route: run under `rocprofv3 --kernel-trace --stats -- python tools/sample_bench.py`.  Needs an MI355X."""
import argparse
import gc
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lrcn_amd  # noqa: E402
from lrcn_amd import lrcn as L  # noqa: E402


def timed(fn, reps):
    fn()   # warm-up: tables, records and pinned staging are allocated by the first call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("N", nargs="?", type=int, default=1024, help="images")
    ap.add_argument("reps", nargs="?", type=int, default=3, help="timed repetitions per line")
    ap.add_argument("--topp", type=float, default=1.0, help="add a nucleus line with this top_p")
    ap.add_argument("--topk", type=int, default=0, help="the added line's top_k (any width; with --topp 1.0 a line of its own from 33 up)")
    ap.add_argument("--nword", type=int, default=30)
    ap.add_argument("--only-nucleus", action="store_true", help="time the --topp / --topk line and its plain-logits base only")
    o = ap.parse_args()
    N, reps = o.N, o.reps
    S, nword, V = 5, o.nword, 10640
    ctx = L.Context(1000, 1000, 1000, V, max_B=N * S, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    fj = L.to_jl((np.random.default_rng(0).standard_normal((N, 4096)) * 0.01).astype(np.float32))
    gc.collect()
    gc.freeze()   # (tools/beam_bench.py: keep full cyclic-GC passes out of the timed decodes)
    routes = [("fused gumbel, top_k 0", "1", 0), ("fused top-K records, top_k 3", "1", 3),
              ("row kernel, top_k 0 (LRCN_DECODE_SMAX=0)", "0", 0), ("row kernel, top_k 10", "1", 10)]
    routes = [(name, knob, k, 1.0) for name, knob, k in routes]
    if o.only_nucleus:
        routes = [r for r in routes if r[1] == "0" or r[2] == 0]
    if o.topp < 1.0 or o.topk > 32:
        routes.append(("nucleus kernel, top_k %d top_p %g" % (o.topk, o.topp), "1", o.topk, o.topp))
    for name, knob, k, p in routes:
        os.environ["LRCN_DECODE_SMAX"] = knob
        dt, out = timed(lambda: L.sample_batch(ctx, param, fj, S, nword, temperature=1.0, top_k=k, seed=1, top_p=p), reps)
        steps = max(len(t) for img in out for t, _ in img) - 1
        print("sample %-42s N=%d S=%d nword=%d  %7.1f ms  %9.0f rows/s  %7.0f captions/s  (%d steps, mean length %.1f)"
              % (name, N, S, nword, dt * 1e3, N * S * steps / dt, N * S / dt, steps, np.mean([len(t) for img in out for t, _ in img])))
    os.environ.pop("LRCN_DECODE_SMAX", None)
    if o.only_nucleus:
        ctx.close()
        return
    dt, out = timed(lambda: L.beam_search_batch(ctx, param, fj, S, nword), reps)
    steps = max(len(t) for t, _ in out) - 1
    print("beam   %-42s N=%d K=%d nword=%d  %7.1f ms  %9.0f rows/s  %7.0f captions/s  (%d steps)"
          % ("width 5 (same rows)", N, S, nword, dt * 1e3, N * S * steps / dt, N / dt, steps))
    ctx.close()


if __name__ == "__main__":
    main()
