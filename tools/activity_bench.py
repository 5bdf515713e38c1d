"""Activity recognition (include/lrcn_activity.h) timing on one GPU: ms per loss_grad + Adam step and per predict at T = 16, F = 4096,
C = 101 (the paper's shape), H = 256 and 1024, B = 32 / 128 / 512 clips, with FLOP rates from the shapes, beside the bf16 VGG forward of
the same B*T frames.  Prints one line per configuration and a JSON summary line.
usage: python tools/activity_bench.py [--dtype bf16|f32] [--iters 20] [--vgg-max 2048] [--drop 0.9,0.5] [--out FILE]
--drop adds train_drop_ms: the same step with seeded dropout on the frame features and the LSTM output, timed in the same process."""
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
from lrcn_amd import activity as A
from lrcn_amd import lrcn as L


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def flops(F, H, C, T, B):
    M = T * B
    fwd = 2.0 * M * (F * 4 * H + H * 4 * H + H * C)          # input projection, recurrence, head
    bwd = 2.0 * M * (H * C * 2 + 4 * H * H * 2 + 4 * H * F)  # dWout + dh, recurrent dh + dW[F:], dW[0:F]
    return fwd, fwd + bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--vgg-max", type=int, default=512, help="largest frame count whose VGG forward is timed directly (above: scaled)")
    ap.add_argument("--drop", metavar="P_IN,P_OUT", help="also time the step with dropout (include/lrcn_act_dropout.h): train_drop_ms")
    ap.add_argument("--out")
    o = ap.parse_args()
    drop = tuple(float(v) for v in o.drop.split(",")) if o.drop else None
    if drop is not None and len(drop) != 2:
        ap.error("--drop takes P_IN,P_OUT")
    dt = lrcn_amd.LRCN_BF16 if o.dtype == "bf16" else lrcn_amd.LRCN_F32
    F, C, T = 4096, 101, 16
    rng = np.random.default_rng(0)
    # VGG forward per frame, measured once at up to vgg_max frames (the forward is throughput-bound from a few hundred images on)
    nv = o.vgg_max
    ctx = L.Context(8, 8, 8, 8, max_B=1, max_T=1, vgg_dtype=lrcn_amd.LRCN_BF16, max_images=nv)
    L.vgg_load(ctx, *L.synthetic_vgg_weights(seed=1))
    img = torch.as_tensor(rng.integers(0, 256, size=(nv, 224, 224, 3), dtype=np.uint8)).cuda()
    vf = L.jl_empty(nv, L.CNNOUT)
    vgg_s = timed(lambda: L.convnet_u8(ctx, img, feats=vf), max(3, o.iters // 4), warm=2)
    vgg_per_frame = vgg_s / nv
    del img
    ctx.close()
    print("vgg bf16 forward: %d frames %.3f ms (%.1f us / frame)" % (nv, vgg_s * 1e3, vgg_per_frame * 1e6), flush=True)
    rows = []
    for H in (256, 1024):
        for B in (32, 128, 512):
            m = A.ActivityModel(F, H, C, max_B=B, max_T=T, dtype=dt, seed=1)
            x = L.to_jl((rng.standard_normal((B * T, F)) * 0.5).astype(np.float32))
            lab = rng.integers(0, C, B).astype(np.int32)
            lens = np.full(B, T, np.int32)
            tr = timed(lambda: (m.loss_grad(x, lab, lens, T), m.adam_step(1e-4)), o.iters)
            pr = timed(lambda: m.predict(x, lens, T), o.iters)
            f_fwd, f_tr = flops(F, H, C, T, B)
            vgg = vgg_per_frame * B * T
            r = {"H": H, "B": B, "T": T, "F": F, "C": C, "dtype": o.dtype, "train_ms": tr * 1e3, "predict_ms": pr * 1e3,
                 "train_tflops": f_tr / tr / 1e12, "predict_tflops": f_fwd / pr / 1e12, "vgg_forward_ms": vgg * 1e3,
                 "train_over_vgg": tr / vgg, "predict_over_vgg": pr / vgg}
            rows.append(r)
            print("H=%4d B=%3d: loss_grad+adam %.3f ms (%.1f TFLOP/s)  predict %.3f ms (%.1f TFLOP/s)  vgg forward of the %d frames %.1f ms"
                  "  -> train %.1f %%, predict %.1f %% of it" % (H, B, tr * 1e3, r["train_tflops"], pr * 1e3, r["predict_tflops"], B * T,
                                                                 vgg * 1e3, 100 * tr / vgg, 100 * pr / vgg), flush=True)
            if drop is not None:   # the same model and batch in the same process, a new seed every step as train_step draws it
                seeds = iter(range(1, 1 << 30))
                plain = lambda: (m.loss_grad(x, lab, lens, T), m.adam_step(1e-4))  # noqa: E731
                dropped = lambda: (m.loss_grad(x, lab, lens, T, pdrop_in=drop[0], pdrop_out=drop[1], drop_seed=next(seeds)),  # noqa: E731
                                   m.adam_step(1e-4))
                # three alternating windows of each, so that the spread between windows of one kind stands beside the difference
                tp, td = [], []
                for _ in range(3):
                    td.append(timed(dropped, o.iters) * 1e3)
                    tp.append(timed(plain, o.iters) * 1e3)
                r.update({"drop": list(drop), "train_drop_ms": float(np.median(td)), "train_drop_ms_windows": td, "train_ms_windows": tp,
                          "train_drop_over_train": float(np.median(td) / np.median(tp))})
                print("            with dropout %g / %g: %.3f ms (windows %s) against %.3f ms (windows %s): %.3f x"
                      % (drop[0], drop[1], np.median(td), " ".join("%.3f" % v for v in td), np.median(tp), " ".join("%.3f" % v for v in tp),
                         np.median(td) / np.median(tp)), flush=True)
            m.close()
            torch.cuda.empty_cache()
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)),
                                         stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    summary = {"tool": "activity_bench", "parent_commit": commit, "vgg_us_per_frame": vgg_per_frame * 1e6, "rows": rows}
    print(json.dumps(summary))
    if o.out:
        with open(o.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
