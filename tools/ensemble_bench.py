#!/usr/bin/env python3
"""Ensemble beam search (lrcn_beam_ensemble_batch, include/lrcn_ensemble.h) at M = 1, 2 and 4 members against M times the single-model
call on the same route: time per call and per decode step.  bf16, E = H = 1000, V = 10640, the decisive random models of
tools/constrained_bench.py (one seed per member), eos improbable so that every call runs all nword + 1 steps.

The single-model line is lrcn_beam_constrained_batch with one banned word that no row proposes: the f32-logits route that every member of
an ensemble runs (the fused softmax / top-K epilogue of the n-best beam at K < 6 is given up by both), so `ensemble / (M x single)` is
like for like.  M = 1 is that call itself (lrcn_ensemble.h) and shows the measurement's own spread.

Every shape is measured in a process of its own, started from here under its own time limit; in it the calls alternate, each timed on the
host around the synchronous C call.  The first child that fails or runs out of time ends the run.  One JSON line per shape; --md writes
the table as well.  Needs an MI355X.

    python tools/ensemble_bench.py [--shapes 512x10 1024x5] [--members 1 2 4] [--iters 7] [--md profiles/ensemble_bench.md]

--mix M runs nothing but the mix kernel (lrcn_ensemble_mix_logits) --mix_calls times per mode, the modes alternating, on M members of
--mix_rows x V logits: the program for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/ensemble_bench.py
--mix 4), whose average kernel time goes over the algorithmic bytes 4 R V (M + 1).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = H = 1000
V = 10640
DEAD = 77   # the single-model line's banned word: its output bias is -30 in every member, no row proposes it


def decisive(L, ctx, seed):
    import torch
    import lrcn_amd
    param = L.initweights(ctx, seed=seed)
    ctx.sync()
    torch.manual_seed(seed)
    with torch.no_grad():   # decisive: W1, W2 x 2, Wout x 16, bout ~ N(0, 2), b1 + N(0, 0.5); eos improbable
        param[0].mul_(2.0)
        param[2].mul_(2.0)
        param[7].mul_(16.0)
        param[8].copy_(torch.randn_like(param[8]) * 2.0)
        param[1].add_(torch.randn_like(param[1]) * 0.5)
        param[8][0, lrcn_amd.EOS] = -30.0
        param[8][0, DEAD] = -30.0
    torch.cuda.synchronize()
    return param


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
    Mmax = max(o.members)
    ctxs = [L.Context(E, H, H, V, max_B=N * K, max_T=1, lstm_dtype=lrcn_amd.LRCN_BF16) for _ in range(Mmax)]
    params = [decisive(L, c, 4 + m) for m, c in enumerate(ctxs)]
    fj = L.to_jl((np.random.default_rng(11).standard_normal((N, 4096)) * 0.05).astype(np.float32))
    # warm-up (tables, lazily allocated state, pinned staging) and the check that no call stops early
    lists = {"single": L.beam_constrained_batch(ctxs[0], params[0], fj, K, o.nword, o.alpha, (DEAD,))}
    for M in o.members:
        lists["M%d" % M] = L.beam_ensemble_batch(ctxs[:M], params[:M], fj, K, o.nword, o.alpha, None, o.mode, (DEAD,) if M == 1 else ())
    for name, imgs in lists.items():
        assert all(len(img) == K and all(len(e[0]) == steps + 1 for e in img) for img in imgs), "%s: an image finished early: per-step times would be off" % name
    for m in range(1, Mmax):   # every member's single-model call has run once as well
        L.beam_constrained_batch(ctxs[m], params[m], fj, K, o.nword, o.alpha, (DEAD,))
    Lh = o.nword + 2
    tok, ln, v1, v2 = (C.c_int32 * (N * K * Lh))(), (C.c_int * (N * K))(), (C.c_float * (N * K))(), (C.c_float * (N * K))()
    p9s, fp = [L._p9(p) for p in params], L._ptr(fj)
    arr = (C.c_int32 * 1)(DEAD)
    cons = _lib.Constraints(arr, 1, 0, 0)
    lib = _lib.lib()

    def ensemble(M):
        hs = (C.c_void_p * M)(*[c._h.value for c in ctxs[:M]])
        ps = (C.c_void_p * M)(*[C.addressof(p) for p in p9s[:M]])
        md = {"prob": 0, "logprob": 1}[o.mode]

        def run():
            _lib.check(ctxs[0]._h, lib.lrcn_beam_ensemble_batch(hs, ps, M, None, md, fp, N, K, 0, 0.0, o.nword, float(o.alpha),
                                                                C.byref(cons) if M == 1 else None, tok, ln, v1, v2))
        return run

    fns = {"single": lambda: ctxs[0]._call("lrcn_beam_constrained_batch", p9s[0], fp, N, K, 0, 0.0, o.nword, float(o.alpha), C.byref(cons), tok, ln, v1, v2)}
    for M in o.members:
        fns["M%d" % M] = ensemble(M)
    gc.collect()
    gc.freeze()   # (tools/beam_bench.py: keep full cyclic-GC passes out of the timed decodes)
    times = {k: [] for k in fns}
    for _ in range(o.iters):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()   # returns after its results are on the host
            times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"images": N, "K": K, "mode": o.mode, "nword": o.nword, "steps": steps, "alpha": o.alpha, "iters": o.iters, "members": o.members}
    for k in fns:
        t = np.array(times[k])
        out[k] = {"ms_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3), "ms_max": round(float(t.max()), 3),
                  "ms_per_step": round(float(np.median(t)) / steps, 4)}
    for M in o.members:
        out["M%d_over_M_single" % M] = round(out["M%d" % M]["ms_median"] / (M * out["single"]["ms_median"]), 4)
    print(json.dumps(out))
    for c in ctxs:
        c.close()
    return 0


def mix_only(o):
    import ctypes as C

    sys.path.insert(0, ROOT)
    import torch
    import lrcn_amd
    from lrcn_amd import lrcn as L

    M, R = o.mix, o.mix_rows
    ctx = L.Context(16, 16, 16, 20, max_B=8, max_T=1, lstm_dtype=lrcn_amd.LRCN_F32)   # the entry does not depend on its sizes
    ld = (V + 63) // 64 * 64   # the decode's own leading dimension
    torch.manual_seed(1)
    zs = [torch.randn((R, ld), dtype=torch.float32, device="cuda") * 8.0 for _ in range(M)]
    out = torch.empty((R, ld), dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * M)(*[z.data_ptr() for z in zs])
    lds = (C.c_int64 * M)(*[ld] * M)
    torch.cuda.synchronize()
    for _ in range(o.mix_calls):   # the two modes alternate: neither has the cold start or the warm end of the run to itself
        for mode in (0, 1):
            ctx._call("lrcn_ensemble_mix_logits", ptrs, lds, M, None, mode, R, V, C.c_void_p(out.data_ptr()), ld)
    ctx.sync()
    print(json.dumps({"mix_members": M, "rows": R, "V": V, "ld": ld, "calls_per_mode": o.mix_calls, "algorithmic_bytes": 4 * R * V * (M + 1)}))
    ctx.close()
    return 0


def table(rows):
    r0 = rows[0]
    lines = ["## Ensemble calls against M single-model calls (tools/ensemble_bench.py)", "",
             "bf16, E = H = 1000, V = 10640, nword %d (%d decode steps, eos improbable: no early stop), alpha %g, mode %s, uniform weights; median "
             "of %d calls each, the calls alternating in one process per shape, host time around the synchronous call.  `single` is "
             "lrcn_beam_constrained_batch of member 0 with one banned word that never binds: the f32-logits route every member runs.  M = 1 is "
             "that call." % (r0["nword"], r0["steps"], r0["alpha"], r0["mode"], r0["iters"]), "",
             "| images | K | rows | call | ms median (min .. max) | ms per step | / (M x single) |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        s = r["single"]
        lines.append("| %d | %d | %d | single | %.3f (%.3f .. %.3f) | %.4f | |" % (r["images"], r["K"], r["images"] * r["K"], s["ms_median"], s["ms_min"],
                                                                                  s["ms_max"], s["ms_per_step"]))
        for M in r["members"]:
            e = r["M%d" % M]
            lines.append("| %d | %d | %d | ensemble M = %d | %.3f (%.3f .. %.3f) | %.4f | %.4f |" %
                         (r["images"], r["K"], r["images"] * r["K"], M, e["ms_median"], e["ms_min"], e["ms_max"], e["ms_per_step"],
                          r["M%d_over_M_single" % M]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["512x10", "1024x5"], help="images x beam width")
    ap.add_argument("--members", nargs="+", type=int, default=[1, 2, 4])
    ap.add_argument("--mode", choices=["prob", "logprob"], default="prob")
    ap.add_argument("--nword", type=int, default=20)
    ap.add_argument("--alpha", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds each shape's process may take")
    ap.add_argument("--md", default="", help="write the table here as well")
    ap.add_argument("--mix", type=int, default=0, help="run the mix kernel alone on this many members (for a kernel trace)")
    ap.add_argument("--mix_rows", type=int, default=5120)
    ap.add_argument("--mix_calls", type=int, default=20)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    o = ap.parse_args()
    if o.mix:
        return mix_only(o)
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
