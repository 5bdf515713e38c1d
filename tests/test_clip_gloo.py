"""CPU, world_size 2 over gloo: dp.py's control flow of device-side gradient-norm clipping (group pipeline and sharded update) with numpy
stand-ins for the device calls (tests/clip_oracle_ops.py).  Two ranks that clip every step equal one process that clips the whole batch's
gradient."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import oracle as orc

import clip_ref
from clip_oracle_ops import ClipOracleOps
from dp_oracle_ops import HostAdam

MAX_NORM = 1e-3   # far below the gradient norm of the golden batch: every step clips (asserted from the reference run below)
STEPS = 2


def _worker(rank, world, port, golden, out, mode):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from lrcn_amd import dp
    z = np.load(golden)
    dims = tuple(int(z[k]) for k in ("E", "H1", "H2", "V"))
    param = [torch.as_tensor(np.array(z["p_" + n])) for n in orc.PARAM_NAMES]
    Bg = z["feats"].shape[0]
    rows = dp.shard_rows(Bg, world, rank)
    ops = ClipOracleOps(dims)
    tr = dp.DataParallelTrainer(None, param, HostAdam(param), Bg, world, rank, pdrop=0.0, ops=ops, shard_adam=(mode == "shard_adam"),
                                gclip=MAX_NORM)
    assert tr.backend == "torch" and tr._dev_clip
    assert tr.shard == (mode == "shard_adam") and (tr.shard or tr._group_pipeline())
    feats = torch.as_tensor(z["feats"][rows])
    toks = z["tokens"][:, rows]
    losses = []
    for _ in range(STEPS):
        tr.step(None, toks, feats=feats)
        losses.append(tr.loss_value())
    st = tr.clip_stats()
    assert st["clipped"] == STEPS and st["steps"] == STEPS and st["skipped"] == 0 and st["last_scale"] < 1.0
    sets = [e for e in ops.log if e[0] == "clip_set"]
    if mode == "group_pipeline":
        # per step: five [wait -> (all-reduce) -> sums of squares of the group] on the group's stream, the join, clip_set(9), ONE clipped update
        per_step = [e for e in ops.log if e[0] != "make_streams"]
        assert len(per_step) == STEPS * 13
        for step in range(STEPS):
            ev = per_step[step * 13:(step + 1) * 13]
            for k in range(5):
                assert ev[2 * k] == ("wait", k, "bucket%d" % k) and ev[2 * k + 1] == ("sumsq_model", k, "bucket%d" % k), ev
            assert ev[10:] == [("join", 5), ("clip_set", 9, None), ("adam_all", step + 1, True)], ev
    else:
        # per step: five slices summed into slots 0..4, clip_set(5) after the join, five clipped slice updates with that step's t
        assert [e[1] for e in sets] == [5] * STEPS
        flats = [e for e in ops.log if e[0] == "adam_flat"]
        assert len(flats) == STEPS * 5 and [e[2] for e in flats] == [1] * 5 + [2] * 5
        assert [e[1] for e in ops.log if e[0] == "sumsq"] == list(range(5)) * STEPS
        assert not [e for e in ops.log if e[0] in ("adam", "adam_all")]
    if rank == 0:
        np.savez(out, losses=np.array(losses), **{n: p.numpy() for n, p in zip(orc.PARAM_NAMES, param)})
    np.savez(out + ".rank%d.npz" % rank, **{n: p.numpy() for n, p in zip(orc.PARAM_NAMES, param)})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["group_pipeline", "shard_adam"])
def test_two_ranks_that_clip_equal_the_full_batch(golden_dir, tmp_path, mode):
    golden = os.path.join(golden_dir, "lstm_mid.npz")
    out = str(tmp_path / "clip.npz")
    port = 31700 + (os.getpid() % 2000) + {"group_pipeline": 0, "shard_adam": 1}[mode]
    mp.spawn(_worker, args=(2, port, golden, out, mode), nprocs=2, join=True)
    got = np.load(out)
    r0, r1 = np.load(out + ".rank0.npz"), np.load(out + ".rank1.npz")
    for n in orc.PARAM_NAMES:
        np.testing.assert_array_equal(r0[n], r1[n], err_msg=n)   # both ranks end with identical parameters
    # single-process reference: the whole batch's gradient, clipped by the nine-slot definition, then Adam on the pre-scaled gradient
    z = np.load(golden)
    dims = tuple(int(z[k]) for k in ("E", "H1", "H2", "V"))
    model = orc.Model(*dims, {n: z["p_" + n] for n in orc.PARAM_NAMES})
    mom = {n: np.zeros_like(model.p[n]) for n in orc.PARAM_NAMES}
    var = {n: np.zeros_like(model.p[n]) for n in orc.PARAM_NAMES}
    ref_losses = []
    for t in range(1, STEPS + 1):
        val, g = orc.loss(model, z["feats"], z["tokens"], want_grad=True)
        ref_losses.append(val)
        pre, norm, scale, skip = clip_ref.clip([g.p[n] for n in orc.PARAM_NAMES], MAX_NORM)
        assert norm > MAX_NORM and scale < 1.0 and not skip
        for n, gs in zip(orc.PARAM_NAMES, pre):
            orc.adam(model.p[n], np.asfortranarray(gs), mom[n], var[n], t)
    # the tolerances of test_dp_gloo.py's comparison of the same two runs without clipping
    np.testing.assert_allclose(got["losses"], ref_losses, rtol=1e-6)
    for n in orc.PARAM_NAMES:
        np.testing.assert_allclose(got[n], model.p[n], rtol=0, atol=3e-6, err_msg=n)
