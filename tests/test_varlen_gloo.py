"""CPU, world_size 2 over gloo: the data-parallel trainer on padded batches of mixed caption lengths.  Every rank passes the GLOBAL batch's
token count as the normaliser (train.shard_block), so two ranks' summed gradients are the single-rank gradients and the parameters after
the steps are the same.  The device operations are CPU stand-ins on tests/varlen_ref.py: this tests the sharding, the normaliser and the
collectives, not the kernels."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from dp_oracle_ops import HostAdam, OracleGroupOps
from oracle import oracle as orc
from varlen_ref import VarlenOracleOps

E, H, V = 12, 16, 23


def blocks_and_feats():
    rng = np.random.default_rng(4)
    blocks, feats = [], {}
    for k, B in enumerate((8, 8, 4)):   # the last window of a split is short
        lens = np.sort(rng.integers(0, 6, size=B)).astype(np.int32)
        lens[-1] = max(int(lens[-1]), 1)
        toks = rng.integers(3, V, size=(int(lens.max()), B)).astype(np.int32)
        for b in range(B):
            toks[lens[b]:, b] = 0
        ids = list(range(100 * k, 100 * k + B))
        for i in ids:
            feats[i] = (rng.standard_normal(4096) * 0.05).astype(np.float32)
        blocks.append((ids, toks, lens))
    return blocks, feats


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from lrcn_amd import dp, train as trn
    blocks, feats = blocks_and_feats()
    m = orc.init_weights(E, H, H, V, seed=5)
    param = [torch.as_tensor(np.array(m.p[n])) for n in orc.PARAM_NAMES]
    optim = HostAdam(param)
    tr = dp.DataParallelTrainer(None, param, optim, 8, world, rank, pdrop=0.0, ops=VarlenOracleOps(OracleGroupOps((E, H, H, V))))

    def feats_of(ids):
        return torch.as_tensor(np.stack([feats[i] for i in ids]))

    # the first step's summed gradients, before any update: one lossgradient per rank, summed over the ranks
    ids, toks, lens, nt = trn.shard_block(blocks[0], world, rank)
    assert nt == int(blocks[0][2].sum()) + len(blocks[0][0])
    tr.ops.lossgradient(param, feats_of(ids), toks, 8, 0.0, 0, tr.grads, lens=lens, norm_tokens=nt)
    g0 = torch.cat([g.reshape(-1).clone() for g in tr.grads])
    if world > 1:
        dist.all_reduce(g0)
    before = trn.average_loss(tr, blocks, feats_of)
    n = 0
    for epoch in (1, 2, 3):
        n += trn.train1(tr, blocks, trn.epoch_order(len(blocks), 3, epoch), feats_of=feats_of)
    after = trn.average_loss(tr, blocks, feats_of)
    assert n * world == 3 * 20
    if rank == 0:
        np.savez(out % world, g0=g0.numpy(), losses=np.asarray([before, after]), step=optim.t, **{"p%d" % k: p.numpy() for k, p in enumerate(param)})
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_on_mixed_lengths_equal_one_rank(tmp_path):
    import socket
    out = str(tmp_path / "vl_w%d.npz")
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
    # float32 per-rank gradients summed against one float32 gradient of the whole batch
    np.testing.assert_allclose(b["g0"], a["g0"], rtol=1e-4, atol=1e-6 * np.abs(a["g0"]).max())
    assert np.abs(a["g0"]).max() > 0
    np.testing.assert_allclose(a["losses"], b["losses"], rtol=1e-6)
    assert a["losses"][1] < a["losses"][0]   # it trains
    for k in range(9):
        np.testing.assert_allclose(a["p%d" % k], b["p%d" % k], rtol=0, atol=2e-6)


def test_the_abi_backend_refuses_padded_batches():
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
    tr = dp.DataParallelTrainer(None, param, HostAdam(param), 4, 1, 0, pdrop=0.0, ops=AbiOps((E, H, H, V)), backend="abi")
    tr.backend, tr._multi = "abi", True   # a one-process stand-in of a multi-rank "abi" job: step() must refuse before any call
    toks = np.zeros((2, 4), np.int32)
    with pytest.raises(LrcnError, match="equal-length"):
        tr.step(None, toks, feats=torch.zeros(4, 4096), lens=np.asarray([2, 1, 1, 0], np.int32))
