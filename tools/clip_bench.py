"""Gradient-norm clipping (include/lrcn_clip.h) on one GPU at the benchmark's workload shape: the trainer's two-stream step from uint8 crops
(VGG-16 forward of step k + 1 on the side stream beside the LSTM step of batch k; E = H = 1000, V = 10640, T = 11, bf16), at 256 rows and
at the 32 rows of a rank of 8.  Three configurations, alternated round by round on one box, each run in a process of its own:

  a  gclip = 0              the plain step
  b  gclip = 5, host path   what the trainer did before the device path: norm of the flat gradient read back by the host
                            (float(vector_norm)), the flat buffer scaled in place, then update! -- selected here by handing the trainer
                            an ops object without the clip methods, which is how dp.py still selects it
  c  gclip = 5, device      sums of squares -> lrcn_clip_set -> clipped update!, no host wait

Prints the per-round step times, their medians, the update segment of lrcn_profile level 2 (one extra pass, not timed) and the shader
clock the box held during the timed steps.  usage: python tools/clip_bench.py [--rounds 3] [--steps 30] [--rows 256 32] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import lrcn_amd
from lrcn_amd import dp
from lrcn_amd import lrcn as L

E = H = 1000
V, T = 10640, 11
CLIP_METHODS = ("grad_sumsq", "clip_set", "clip_slots", "clip_stats")


class HostClipOps:
    """dp.HipOps without the clip methods: the trainer then clips on the host, as it did before include/lrcn_clip.h."""

    def __init__(self, ctx):
        self._ops = dp.HipOps(ctx)

    def __getattr__(self, name):
        if name in CLIP_METHODS:
            raise AttributeError(name)
        return getattr(self._ops, name)


def make(rows, gclip, host):
    ctx = L.Context(E, H, H, V, max_B=rows, max_T=T, lstm_dtype=lrcn_amd.LRCN_BF16, vgg_dtype=lrcn_amd.LRCN_BF16, max_images=rows)
    L.vgg_load(ctx, *L.synthetic_vgg_weights(seed=1))
    param = L.initweights(ctx, seed=42)
    tr = dp.DataParallelTrainer(ctx, param, L.initparams(param), rows, 1, 0, pdrop=0.4, seed=7, gclip=gclip, rows=rows,
                                ops=HostClipOps(ctx) if host else None)
    assert tr._dev_clip == (gclip > 0 and not host)
    return ctx, tr


def run(tr, imgs, toks, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(n):
        tr.step(imgs[k % 2], toks, next_img_u8=imgs[(k + 1) % 2])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def one(cfg, rows, steps, gclip):
    """One configuration in this process: 10 warm-up steps, `steps` timed ones, then as many under lrcn_profile level 2 for the update segment."""
    from bench import HwSampler
    rng = np.random.default_rng(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    imgs = [torch.randint(0, 256, (rows, 224, 224, 3), generator=g, device="cuda", dtype=torch.uint8) for _ in range(2)]
    toks = torch.as_tensor(rng.integers(3, V, size=(T, rows)).astype(np.int32)).cuda()
    ctx, tr = make(rows, 0.0 if cfg == "a" else gclip, cfg == "b")
    hw = HwSampler(torch.cuda.current_device())
    run(tr, imgs, toks, 10)
    hw.start()
    ms = run(tr, imgs, toks, steps)
    clock = hw.stop()
    L.profile(ctx, 2)   # event pairs around update! alone (c: the sums of squares and lrcn_clip_set are outside it)
    run(tr, imgs, toks, steps)
    u = L.profile_segments(ctx)["update"]
    L.profile(ctx, 0)
    st = tr.clip_stats()
    tr.close()
    ctx.close()
    return {"cfg": cfg, "rows": rows, "step_ms": ms, "update_segment_us": u[0] / max(u[1], 1) * 1e3, "clip_stats": st,
            "sclk_mhz": (clock.get("sclk_mhz") or {}).get("median") if clock.get("available") else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--gclip", type=float, default=5.0)
    ap.add_argument("--one", choices=["a", "b", "c"], help="(internal) run this configuration here and print its JSON line")
    ap.add_argument("--out")
    o = ap.parse_args()
    if o.one:
        print("RESULT " + json.dumps(one(o.one, o.rows[0], o.steps, o.gclip)), flush=True)
        return 0
    # One process per (round, configuration): three trainers alive in one process share HIP's few hardware queues, and a side stream that
    # lands on the main stream's queue runs the VGG forward in order with the LSTM step (dp.streams_share_a_queue) -- every configuration
    # gets the stream-to-queue mapping of a fresh process instead.  This parent never opens the GPU.
    results = []
    for rows in o.rows:
        runs = {k: [] for k in "abc"}
        for _ in range(o.rounds):
            for k in "abc":
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", k, "--rows", str(rows), "--steps", str(o.steps),
                                    "--gclip", str(o.gclip)], stdout=subprocess.PIPE, text=True, timeout=300)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(p.stdout)
                    raise SystemExit("configuration %s at %d rows ended with status %d: nothing more is started" % (k, rows, p.returncode))
                runs[k].append(json.loads(line[0][7:]))
        r = {"rows": rows, "runs": runs, "median_ms": {k: float(np.median([x["step_ms"] for x in v])) for k, v in runs.items()},
             "update_segment_us": {k: float(np.median([x["update_segment_us"] for x in v])) for k, v in runs.items()},
             "sclk_mhz": sorted(x["sclk_mhz"] for v in runs.values() for x in v if x["sclk_mhz"] is not None)}
        results.append(r)
        print("rows %3d: " % rows + "  ".join("%s %.3f ms (rounds %s; update! %.1f us)" % (k, r["median_ms"][k], " ".join("%.3f" % x["step_ms"] for x in runs[k]),
                                                                                          r["update_segment_us"][k]) for k in "abc")
              + "  sclk %s MHz" % (("%.0f..%.0f" % (r["sclk_mhz"][0], r["sclk_mhz"][-1])) if r["sclk_mhz"] else "n/a"), flush=True)
    try:
        commit = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    summary = {"tool": "clip_bench", "commit": commit, "E": E, "H": H, "V": V, "T": T, "dtype": "bf16", "gclip": o.gclip, "steps": o.steps,
               "results": results}
    print(json.dumps(summary))
    if o.out:
        with open(o.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
