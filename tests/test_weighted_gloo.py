"""CPU, world_size 2 over gloo: DataParallelTrainer.step(row_weights=) on padded batches.  Each rank passes its own rows' weights and the
GLOBAL batch's token count, so two ranks' summed gradients are the single-rank gradients and the parameters after the steps are the same.
The device operations are CPU stand-ins on tests/weighted_ref.py: this tests the sharding, the normaliser and the collectives, not the
kernels."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dp_oracle_ops import HostAdam, OracleGroupOps
from oracle import oracle as orc
from weighted_ref import WeightedOracleOps

E, H, V = 12, 16, 23


def blocks():
    """(feats [B][4096], tokens [T][B], lens [B], weights [B]) per step; rows, weights and lengths differ between the two halves."""
    rng = np.random.default_rng(9)
    out = []
    for B in (8, 8, 4):
        lens = rng.integers(0, 6, size=B).astype(np.int32)
        lens[0], lens[-1] = 0, 5
        toks = rng.integers(3, V, size=(5, B)).astype(np.int32)
        w = rng.standard_normal(B).astype(np.float32)
        w[1], w[B // 2] = 0.0, -abs(w[B // 2]) - 0.1     # a zero and a negative weight, one in each rank's half
        feats = (rng.standard_normal((B, 4096)) * 0.05).astype(np.float32)
        out.append((feats, toks, lens, w))
    return out


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from lrcn_amd import dp
    m = orc.init_weights(E, H, H, V, seed=5)
    param = [torch.as_tensor(np.array(m.p[n])) for n in orc.PARAM_NAMES]
    optim = HostAdam(param)
    tr = dp.DataParallelTrainer(None, param, optim, 8, world, rank, pdrop=0.0, ops=WeightedOracleOps(OracleGroupOps((E, H, H, V))))
    g0 = None
    for epoch in range(3):
        for feats, toks, lens, w in blocks():
            B = len(lens)
            nt = int(lens.sum()) + B                                  # the global batch's count, on every rank
            rows = slice(rank * B // world, (rank + 1) * B // world)  # this rank's rows
            f, t, n, ww = torch.as_tensor(feats[rows]), np.ascontiguousarray(toks[:, rows]), lens[rows], w[rows]
            if g0 is None:   # the first step's summed gradients, before any update
                tr.ops.lossgradient(param, f, t, 8, 0.0, 0, tr.grads, lens=n, norm_tokens=nt, row_weights=ww)
                g0 = torch.cat([g.reshape(-1).clone() for g in tr.grads])
                if world > 1:
                    dist.all_reduce(g0)
            tr.step(None, t, feats=f, lens=n, norm_tokens=nt, row_weights=ww)
    if rank == 0:
        np.savez(out % world, g0=g0.numpy(), step=optim.t, **{"p%d" % k: p.numpy() for k, p in enumerate(param)})
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_with_row_weights_equal_one_rank(tmp_path):
    import socket
    out = str(tmp_path / "w_w%d.npz")
    for world in (1, 2):
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        if world == 1:
            _worker(0, 1, port, out)
        else:
            mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    a, b = np.load(out % 1), np.load(out % 2)
    assert int(a["step"]) == int(b["step"]) == 9
    # the tolerances of tests/test_varlen_gloo.py: float32 per-rank gradients summed against one float32 gradient of the whole batch
    np.testing.assert_allclose(b["g0"], a["g0"], rtol=1e-4, atol=1e-6 * np.abs(a["g0"]).max())
    assert np.abs(a["g0"]).max() > 0
    for k in range(9):
        np.testing.assert_allclose(a["p%d" % k], b["p%d" % k], rtol=0, atol=2e-6)


def test_row_weights_need_lens_and_the_abi_backend_refuses_them():
    import pytest
    from lrcn_amd import dp
    from lrcn_amd.lrcn import LrcnError

    class AbiOps(OracleGroupOps):
        def train_step_dp(self, *a, **k):
            raise AssertionError("must not be reached")

        def comm_probe(self):
            return True, ""

    m = orc.init_weights(E, H, H, V, seed=5)
    param = [torch.as_tensor(np.array(m.p[n])) for n in orc.PARAM_NAMES]
    toks, w = np.zeros((2, 4), np.int32), np.ones(4, np.float32)
    tr = dp.DataParallelTrainer(None, param, HostAdam(param), 4, 1, 0, pdrop=0.0, ops=WeightedOracleOps(OracleGroupOps((E, H, H, V))))
    with pytest.raises(LrcnError, match="lens"):
        tr.step(None, toks, feats=torch.zeros(4, 4096), row_weights=w)
    tr = dp.DataParallelTrainer(None, param, HostAdam(param), 4, 1, 0, pdrop=0.0, ops=AbiOps((E, H, H, V)), backend="abi")
    tr.backend, tr._multi = "abi", True   # a one-process stand-in of a multi-rank "abi" job: step() must refuse before any call
    with pytest.raises(LrcnError, match="equal-length"):
        tr.step(None, toks, feats=torch.zeros(4, 4096), lens=np.asarray([2, 1, 1, 0], np.int32), row_weights=w)
