"""Data-parallel training on the host: the sharded dataset, the arithmetic of the ranks' loss shares in plain torch (float64) with a fake
two-rank reducer, ``distributed.Reducer`` on a world-2 gloo group, and the loop's rank-0-only side effects with stub steps."""
import ctypes
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from hpe_amd import ops
from hpe_amd.distributed import shard_bounds
from hpe_amd.records import RecordDataset, write_tfrecords
from hpe_amd.trainer import rank_zero_only, run_training_loop
from oracle import hmr_oracle as O


# ---------------------------------------------------------------------- RecordDataset(shard=)
@pytest.mark.parametrize("G,world", [(4, 2), (3, 2), (5, 3)])
def test_sharded_dataset_covers_the_global_batches(tmp_path, G, world):
    path = str(tmp_path / "r.tfrecords")
    assert write_tfrecords(path, [b"record-%03d" % i for i in range(13)]) == 13
    parsed = []

    def parse(p):
        parsed.append(p)
        return p

    whole = RecordDataset(path, G, shuffle_seed=5, parse=lambda p: p)
    ranks = [RecordDataset(path, G, shuffle_seed=5, parse=parse, shard=(r, world)) for r in range(world)]
    seen = []
    for _ in range(2):  # two passes: two permutations, the same on every rank
        want = list(whole)
        got = [list(d) for d in ranks]
        assert len(want) == 13 // G and all(len(g) == len(want) for g in got)
        for b, batch in enumerate(want):
            assert [len(g[b]) for g in got] == [shard_bounds(G, r, world)[1] - shard_bounds(G, r, world)[0] for r in range(world)]
            assert sum((g[b] for g in got), []) == batch
        seen.append(want)
    assert seen[0] != seen[1]
    assert len(parsed) == 2 * (13 // G) * G  # each record parsed by exactly one rank: the slice is cut before parse
    # rows that stay together: 2 * G rows in units of 2
    pairs = [list(RecordDataset(path, 2 * G, parse=lambda p: p, shard=(r, world), shard_unit=2)) for r in range(world)]
    plain = list(RecordDataset(path, 2 * G, parse=lambda p: p))
    for b, batch in enumerate(plain):
        assert sum((p[b] for p in pairs), []) == batch
        assert [len(p[b]) for p in pairs] == [2 * (shard_bounds(G, r, world)[1] - shard_bounds(G, r, world)[0]) for r in range(world)]
    with pytest.raises(ValueError):
        RecordDataset(path, G, shard=(world, world))
    with pytest.raises(ValueError):
        RecordDataset(path, 3, shard=(0, 2), shard_unit=2)


# ---------------------------------------------------------------------- the shares, in float64, two ranks with rows 2 + 1
class FakeTwoRanks(object):
    """what an all-reduce leaves on every rank: the sum of the ranks' blocks"""

    def __init__(self):
        self.calls = 0

    def sum(self, blocks):
        self.calls += 1
        total = sum(blocks)
        return [total.clone() for _ in blocks]


SHARDS = [(0, 2), (2, 3)]
TOL = 1e-13  # float64 sums of at most a few hundred terms, taken in another order: n * 2^-53 stays below it


def _kp_parts(kp_gt, kp_pred):
    vis = kp_gt[..., 2:3]
    return (vis * (kp_pred - kp_gt[..., :2]).abs()).sum(), 2.0 * torch.count_nonzero(vis).to(kp_gt.dtype)


@pytest.mark.parametrize("blind", [None, 0, 1, "all"])
def test_kp_shares_add_up(blind):
    """blind: the shard (or all of them) without one visible keypoint"""
    g = torch.Generator().manual_seed(3)
    kp_gt = torch.cat([torch.rand(3, 19, 2, generator=g, dtype=torch.float64) * 2 - 1,
                       (torch.rand(3, 19, 1, generator=g) > 0.3).double()], 2)
    kp_pred = torch.rand(3, 19, 2, generator=g, dtype=torch.float64) * 2 - 1
    for r, (lo, hi) in enumerate(SHARDS):
        if blind == "all" or blind == r:
            kp_gt[lo:hi, :, 2] = 0.0
    ref = float(O.kp_reprojection_loss(kp_gt.numpy(), kp_pred.numpy()))
    parts = [_kp_parts(kp_gt[lo:hi], kp_pred[lo:hi]) for lo, hi in SHARDS]
    red = FakeTwoRanks()
    counts = red.sum([p[1].reshape(1) for p in parts])  # before the forward: one all-reduce of the count
    shares = [ops.kp_loss_share(p[0], c) for p, c in zip(parts, counts)]
    assert red.calls == 1
    assert abs(float(sum(shares)) - ref) <= TOL * max(1.0, abs(ref))
    if blind == "all":
        assert float(sum(shares)) == 0.0 and ref == 0.0
    elif blind is not None:
        assert float(shares[blind]) == 0.0


def test_critic_term_shares_add_up():
    scores = torch.randn(3, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    ref = -scores.mean(0).sum()
    shares = [ops.critic_term_share(scores[lo:hi], 3) for lo, hi in SHARDS]
    assert abs(float(sum(shares) - ref)) <= TOL


def test_wgan_and_penalty_from_reduced_sums():
    """the packed block of (wgan_sums, grad_sums, N) through one all-reduce: wgan, penalty and loss of the single batch, and tangents
    that equal d(gp_weight * penalty) / d(the gradient of any row) of the single batch, taken by autograd"""
    g = torch.Generator().manual_seed(5)
    gp = 10.0
    diff = torch.randn(3, 3, generator=g, dtype=torch.float64)  # fake - real scores per row
    shapes = [(13, 13), (14, 3), (10,), (23, 3, 3)]
    grads = [torch.randn((3,) + s, generator=g, dtype=torch.float64).requires_grad_(True) for s in shapes]
    penalty = ops.critic_gradient_penalty(grads)
    wgan = diff.mean(0).sum()
    (gp * penalty).backward()
    single = ops.wgan_terms(diff.sum(0), [t.detach().sum(0) for t in grads], 3, gp)
    assert abs(float(single["wgan"] - wgan)) <= TOL and abs(float(single["penalty"] - penalty.detach())) <= TOL
    blocks = [ops.pack_critic_sums(diff[lo:hi].sum(0), [t.detach()[lo:hi].sum(0) for t in grads], hi - lo) for lo, hi in SHARDS]
    red = FakeTwoRanks()
    reduced = red.sum(blocks)
    assert red.calls == 1
    for (lo, hi), block in zip(SHARDS, reduced):
        ws, gs, rows = ops.unpack_critic_sums(block, [t.detach()[lo:hi].sum(0) for t in grads])
        assert float(rows) == 3.0 and all(a.shape == torch.Size(s) for a, s in zip(gs, shapes))
        t = ops.wgan_terms(ws, gs, 3, gp)
        for k in ("wgan", "penalty", "loss"):
            assert abs(float(t[k] - single[k])) <= TOL * max(1.0, abs(float(single[k]))), k
        for tan, full in zip(t["tangents"], grads):
            for n in range(3):  # the same vector for every row of every rank
                assert float((tan - full.grad[n]).abs().max()) <= TOL * float(full.grad[n].abs().max())


# ---------------------------------------------------------------------- Reducer and the loop's side effects on a world-2 gloo group
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from hpe_amd import distributed as D

    red = D.Reducer.from_env(backend="gloo", timeout_s=60, device="cpu")
    assert (red.rank, red.world, red.backend, red.active) == (rank, world, "gloo", True)
    out = {}
    grad = torch.full((1000,), float(rank + 1))
    assert red.sum_grad(grad) is grad
    out["grad"] = [float(grad.min()), float(grad.max())]
    block = torch.tensor([1.0, 10.0 * rank, 2.0 - rank], dtype=torch.float64)
    red.sum_block(block)
    out["block"] = block.tolist()
    t = torch.arange(4, dtype=torch.float32) + 100 * rank
    red.broadcast(t)
    out["broadcast"] = t.tolist()
    # the callback, through ctypes as the library calls it, on host memory
    buf = (ctypes.c_double * 6)(*[float(rank + i) for i in range(6)])
    rc = red.callback(None, ctypes.addressof(buf), 6, None)
    out["hook"] = [rc, list(buf)]
    red.reraise()  # nothing kept
    # a callback that raises: caught and kept, nonzero, raised once by reraise()
    real, D.device_doubles = D.device_doubles, lambda *a: (_ for _ in ()).throw(RuntimeError("boom on rank %d" % rank))
    try:
        rc = red.callback(None, ctypes.addressof(buf), 6, None)
    finally:
        D.device_doubles = real
    try:
        red.reraise()
        raised = None
    except RuntimeError as e:
        raised = str(e)
    red.reraise()
    out["raise"] = [rc, raised]
    out["counts"] = red.counts
    # the loop with stub steps: only rank 0 saves and summarises, every rank waits at the barrier of a save
    events = []
    side = rank_zero_only(rank, barrier=red.barrier, save=lambda epoch: events.append("save %d" % epoch), log=lambda m: events.append("log"),
                          after_train_step=lambda s, r: events.append("step %d" % s), after_epoch=lambda e: events.append("epoch %d" % e),
                          after_val_step=None)
    counts = run_training_loop(iter([(i, None, None) for i in range(8)]), lambda g, c: g, num_images=4, batch_size=2, max_epoch=4, save_every=2,
                               summarize=lambda e, tr, va: "line", **side)
    out["loop"], out["events"] = counts, events
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(out, f)
    red.barrier()
    torch.distributed.destroy_process_group()


def test_reducer_and_rank_zero_side_effects_on_gloo(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(tmp_path / ("rank%d.json" % k))) for k in range(2)]
    for k in range(2):
        assert r[k]["grad"] == [3.0, 3.0]
        assert r[k]["block"] == [2.0, 10.0, 3.0]
        assert r[k]["broadcast"] == [0.0, 1.0, 2.0, 3.0]
        assert r[k]["hook"] == [0, [2.0 * i + 1.0 for i in range(6)]]
        assert r[k]["raise"] == [1, "boom on rank %d" % k]
        assert r[k]["counts"] == {"hook": 2, "grad": 1, "block": 1, "broadcast": 1}
        assert r[k]["loop"] == {"steps": 8, "epochs": 4, "saved": [2, 4], "validations": 0}
    assert [e for e in r[0]["events"] if e.startswith("save")] == ["save 2", "save 4"]
    assert sum(e.startswith("step") for e in r[0]["events"]) == 8 and sum(e.startswith("epoch") for e in r[0]["events"]) == 4
    assert "log" in r[0]["events"]
    assert r[1]["events"] == []  # no save, no summary hook, no log line


def test_rank_zero_only_without_a_group():
    """rank 0 of one: everything passes through; no save given, none made up"""
    seen = []
    side = rank_zero_only(0, save=lambda e: seen.append(e), log=seen.append, after_epoch=None, after_train_step=lambda s, r: None)
    assert set(side) == {"log", "save", "after_train_step"}
    side["save"](3)
    assert seen == [3]
    assert "save" not in rank_zero_only(1, log=print)


def test_identity_without_a_group():
    from hpe_amd import distributed as D

    red = D.Reducer(device="cpu")
    assert (red.rank, red.world, red.active) == (0, 1, False)
    t = torch.ones(3)
    assert red.sum_grad(t) is t and red.sum_block(t) is t and red.broadcast(t) is t and t.tolist() == [1.0, 1.0, 1.0]
    red.barrier()
    buf = (ctypes.c_double * 2)(1.0, 2.0)
    assert red.callback(None, ctypes.addressof(buf), 2, None) == 0 and list(buf) == [1.0, 2.0]
    assert np.isfinite(D.DEFAULT_TIMEOUT_S)
