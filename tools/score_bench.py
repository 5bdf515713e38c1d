#!/usr/bin/env python3
"""Caption scoring throughput (lrcn_score_matrix, include/lrcn_score.h) at the retrieval shape of a Flickr30k test split, 1 GPU: 1000 images x
5000 captions (lengths 8 .. 20 from a fixed seeded draw), E = H = 1000, V = 10640, bf16, random weights (initweights) and features, max_B = 5120
pair rows per piece.  One line per route of the logits -- the GEMM_OUT_SMAX_PICK epilogue (fused) and plain logits + k_softmax_xent
(LRCN_SCORE_FUSED=0) -- and one for a matrix of ONE image (LSTM-1 and P = h1 Wproj for all 5000 captions, plus that image's pair steps);
the caption side alone is estimated from it by subtracting 1/N of the fused matrix's time.  pairs/s = N x M / s; TFLOP/s counts the algorithmic per-pair-step work 2 H2 4H2 + 2 h 4H2 + 2 H2 V (~33 MFLOP) over
sum_m (L_m + 1) steps per image.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/score_bench.py`.  Needs an MI355X."""
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
    fn()   # warm-up: tables, records and the scoring arena are allocated by the first call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    M = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    E = H = 1000
    V, h = 10640, 500
    rng = np.random.default_rng(0)
    lens = rng.integers(8, 21, size=M)
    caps = [list(rng.integers(3, V, size=int(n))) for n in lens]
    steps = float(np.sum(lens + 1))
    flop_step = 2 * H * 4 * H + 2 * h * 4 * H + 2 * H * V
    ctx = L.Context(E, H, H, V, max_B=5120, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16)
    param = L.initweights(ctx, seed=42)
    fj = L.to_jl((rng.standard_normal((N, 4096)) * 0.01).astype(np.float32))
    f1 = L.to_jl((rng.standard_normal((1, 4096)) * 0.01).astype(np.float32))
    gc.collect()
    gc.freeze()
    dt1, _ = timed(lambda: L.score_matrix(ctx, param, f1, caps), reps)
    cap_flop = 2.0 * V * E * 4 * H + steps * (2 * H * 4 * H + 2 * H * h)   # T1 once, then the LSTM-1 gate GEMM and Wproj per caption step
    print("score caption side + one image's pairs (1 x %d)       %8.1f ms  (caption-side work %.2f TFLOP; pair work %.2f TFLOP)"
          % (M, dt1 * 1e3, cap_flop / 1e12, steps * flop_step / 1e12))
    res, res_t = {}, {}
    for name, knob in (("fused (GEMM_OUT_SMAX_PICK)", "1"), ("unfused (LRCN_SCORE_FUSED=0)", "0")):
        os.environ["LRCN_SCORE_FUSED"] = knob
        dt, s = timed(lambda: L.score_matrix(ctx, param, fj, caps), reps)
        res[name], res_t[name] = s, dt
        print("score %-32s N=%d M=%d  %9.1f ms  %10.0f pairs/s  %6.1f TFLOP/s  (%.0f pair-steps, %.2f PFLOP)"
              % (name, N, M, dt * 1e3, N * M / dt, N * steps * flop_step / dt / 1e12, N * steps, N * steps * flop_step / 1e15))
    os.environ.pop("LRCN_SCORE_FUSED", None)
    dtf = res_t["fused (GEMM_OUT_SMAX_PICK)"]
    print("caption side alone, estimated as the 1-image call minus 1/N of the fused matrix: %.1f ms (%.0f TFLOP/s)"
          % ((dt1 - dtf / N) * 1e3, cap_flop / max(dt1 - dtf / N, 1e-9) / 1e12))
    a, b = res.values()
    print("fused vs unfused: max |diff| / (L + 1) = %.3g" % float(np.max(np.abs(a - b) / (lens + 1.0)[None, :])))
    ctx.close()


if __name__ == "__main__":
    main()
