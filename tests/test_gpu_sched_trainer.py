"""GPU: scheduled sampling (include/lrcn_sched.h) through the trainer and the command line -- DataParallelTrainer.step(..., sched=) against
lrcn.train_step(..., sched=), and `tools/lrcn.py --train --varlen --ss_start ...` on the tiny dataset of the existing driver tests."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

import lrcn_amd
from lrcn_amd import _lib, dp
from lrcn_amd import lrcn as L
from oracle import oracle as orc

from test_gpu_cli import _epoch_losses, _scene_dataset

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def same_parameters(got, param):
    """The trainer updates through LRCN_OPT_FUSED_UPDATE's Adam kernel, train_step on a plain context through the other one: their
    last-bit differences stay below 1e-8 per step and Adam turns a last-bit gradient difference into a fraction of lr = 1e-3, so the
    project compares the two at atol 2e-5 (tests/test_gpu_fused_update.py).  Another dropout seed, row0, normaliser or set of fed words
    moves a parameter by about lr per step."""
    worst = 0.0
    for n, a, p in zip(orc.PARAM_NAMES, got, param):
        b = L.from_jl(p)
        if a.size:
            worst = max(worst, float(np.abs(a - b).max()))
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-5, err_msg=n)
    print("trainer against train_step: largest parameter difference", worst)


def test_trainer_step_with_sched_is_train_step_with_sched():
    B, T, E, H, V = 12, 5, 64, 64, 131
    rng = np.random.default_rng(4)
    m = orc.init_weights(E, H, H, V, seed=5)
    feats = L.to_jl((rng.standard_normal((B, 4096)) * 0.02).astype(np.float32))
    tokens = rng.integers(3, V, size=(T, B)).astype(np.int32)
    lens = rng.integers(0, T + 1, size=B).astype(np.int32)
    ctx = L.Context(E, H, H, V, max_B=B, max_T=T, lstm_dtype=lrcn_amd.LRCN_F32)
    ctx.set_option(_lib.LRCN_OPT_DETERMINISTIC, 1)
    nt = int(lens.sum()) + B

    pa = L.model_from_arrays(m.p)
    oa = L.initparams(pa)
    tr = dp.DataParallelTrainer(ctx, pa, oa, B, 1, 0, pdrop=0.4, seed=7)
    fed_counts = []
    for k in range(3):
        tr.step(None, tokens, feats=feats, lens=lens, sched=(0.5, 1.0, 100 + k))
        fed_counts.append(L.sched_stats(ctx))
    ctx.sync()
    got = [L.from_jl(p).copy() for p in tr.param]
    tr.close()

    pb = L.model_from_arrays(m.p)
    ob = L.initparams(pb)
    grads = [L.jl_empty(*t.shape) for t in pb]
    for k in range(3):
        L.train_step(ctx, pb, ob, grads, feats, tokens, pdrop=0.4, seed=(7 + k + 1) * 65536, lens=lens, norm_tokens=nt, sched=(0.5, 1.0, 100 + k, 0))
        assert L.sched_stats(ctx) == fed_counts[k]
    assert oa.t == ob.t == 3 and all(e == int(lens.sum()) and 0 < d < e for e, d in fed_counts)
    same_parameters(got, pb)
    assert any(np.abs(a - m.p[n]).max() > 0 for n, a in zip(orc.PARAM_NAMES, got) if a.size)
    # equal-length rows: lens defaults to T, the normaliser to B_global (T + 1)
    pc, pd = L.model_from_arrays(m.p), L.model_from_arrays(m.p)
    oc, od = L.initparams(pc), L.initparams(pd)
    tr = dp.DataParallelTrainer(ctx, pc, oc, B, 1, 0, pdrop=0.0, seed=7)
    tr.step(None, tokens, feats=feats, sched=L.Sched(1.0, 0.0, 5))
    ctx.sync()
    got = [L.from_jl(p).copy() for p in tr.param]
    tr.close()
    L.train_step(ctx, pd, od, grads, feats, tokens, pdrop=0.0, sched=(1.0, 0.0, 5), norm_tokens=B * (T + 1))
    same_parameters(got, pd)
    ctx.close()


def test_cli_scheduled_sampling_logs_eps_and_the_realised_rate(tmp_path, capsys):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    cli = importlib.import_module("lrcn")
    tr, fp, _ = _scene_dataset(tmp_path)
    common = ["--coco", "--datafiles", tr, tr, "--features", fp, fp, "--hidden", "64", "64", "--embed", "64", "--batchsize", "16", "--atype", "f32",
              "--seed", "3", "--train", "--lr", "0.01", "--dropout", "0.2", "--epochs", "2"]
    ss = ["--ss_start", "1", "--ss_every", "1", "--ss_step", "0.5", "--ss_max", "0.5"]

    def sched_lines(out):
        rows = re.findall(r"^\(:sched, (\d+), :eps, ([0-9.e+-]+), :drawn, (\d+), :eligible, (\d+), :rate, ([0-9.]+)\)$", out, flags=re.M)
        return [(int(a), float(b), int(c), int(d), float(e)) for a, b, c, d, e in rows]

    for extra in (["--varlen"], []):   # padded batches, and the equal-length batcher (lens = T)
        assert cli.main(common + ss + extra) == 0
        out = capsys.readouterr().out
        losses = _epoch_losses(out)
        assert len(losses) == 2 and np.isfinite(losses).all(), out
        rows = sched_lines(out)
        assert len(rows) == 2, out
        (e0, eps0, drawn0, elig0, rate0), (e1, eps1, drawn1, elig1, rate1) = rows
        assert (e0, eps0, drawn0, rate0) == (0, 0.0, 0, 0.0) and (e1, eps1) == (1, 0.5)
        assert elig1 >= 100 and abs(rate1 - drawn1 / elig1) <= 1e-4
        # a binomial count of elig1 coins at eps 0.5: three standard deviations
        assert abs(drawn1 - 0.5 * elig1) <= 3 * np.sqrt(elig1 * 0.25), rows
    # off by default: no line, nothing drawn
    assert cli.main(common + ["--varlen"]) == 0
    assert not sched_lines(capsys.readouterr().out)
    with pytest.raises(SystemExit):
        cli.main([a for a in common if a != "--train"] + ss)   # without --train
