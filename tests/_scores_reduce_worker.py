"""Ranks of tests/test_eval_scores_cpu.py::test_scores_reduce_on_gloo_world2: rank r adds batch r of ``made_up_batches`` to a
``metrics.Scores``, reduces it over a world-2 ``gloo`` group on the CPU and writes its sums and its result."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def made_up_batches(n_batches=2, n_stage=3, K=19, seed=3):
    """per batch (counts [n_stage,B,4], kp_err [n_stage,B,K], norm [B,2]) with an empty union, invisible joints and invalid
    normalisers among them; batch b has b + 2 images"""
    g = np.random.Generator(np.random.Philox(seed))
    out = []
    for b in range(n_batches):
        B = b + 2
        counts = g.integers(0, 2000, (n_stage, B, 4)).astype(np.int32)
        counts[:, 0, :3] = 0  # neither a silhouette nor a mask
        err = g.uniform(0.0, 30.0, (n_stage, B, K)).astype(np.float32)
        err[:, :, 3] = -1.0
        err[:, B - 1, 7:] = -1.0
        norm = g.uniform(20.0, 60.0, (B, 2)).astype(np.float32)
        norm[0, b % 2] = -1.0
        out.append((counts, err, norm))
    return out


def worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch

    from hpe_amd import distributed as D, metrics

    red = D.Reducer.from_env(backend="gloo", timeout_s=60, device="cpu")
    assert (red.rank, red.world, red.active) == (rank, world, True)
    s = metrics.Scores().add(*made_up_batches()[rank])
    assert s.reduce(red) is s and red.counts["block"] == 1  # every sum in ONE collective
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump({"sums": s.sums.tolist(), "result": s.result(), "stages": len(s.results())}, f)
    red.barrier()
    torch.distributed.destroy_process_group()
