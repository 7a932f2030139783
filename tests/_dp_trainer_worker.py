"""Child process of tests/test_gpu_data_parallel.py: hpe_amd.Trainer under a process group, on synthetic full-size weights and one fixed
batch of G = 2 images, with fixed dropout masks and interpolation draws.

    world1 PORT OUT        no group, then a world-1 ``nccl`` group with HPE_FORCE_DIST=1: two train_steps each, bit for bit the same
    world2 RANK PORT OUT   rank RANK of a world-2 ``gloo`` group, both ranks on GPU 0: row RANK of the batch, two train_steps; the
                           replicas' tensors are compared after every step, step 1's losses and thetas are written for the parent
"""
import hashlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import synthetic  # noqa: E402
from hpe_amd.augment import mocap_real  # noqa: E402

G, STAGES, STEPS = 2, 3, 2
HOOKS_PER_STEP = 53 + 2 * 53  # the training forward, then the backward with its own forward


_ASSETS = {}


def make_trainer():
    if not _ASSETS:  # generated once: world1 builds two trainers
        w = dict(synthetic.make_encoder_params())
        w.update(synthetic.make_regressor_params(variant="bounded"))
        w.update(synthetic.make_critic_params())
        _ASSETS.update(weights=w, smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params())
    cfg = types.SimpleNamespace(batch_size=G, epoch=1, checkpoint_dir=None, use_validation=False, **_ASSETS)
    return hpe_amd.Trainer(cfg, [], [], log=lambda s: None, generator=torch.Generator(device="cuda").manual_seed(1))


def make_inputs(engine):
    """the GLOBAL batch: images, kp_gt, the real triple of G * STAGES rows (stage-major, as the critic concatenates the stages), and per
    step the dropout masks [2,G,1024] and the interpolation draws of the G * STAGES rows"""
    g = torch.Generator().manual_seed(4)
    images = torch.from_numpy(synthetic.make_images(G, seed=13)).cuda()
    kp = torch.cat([torch.rand(G, 19, 2, generator=g) * 1.2 - 0.6, (torch.rand(G, 19, 1, generator=g) > 0.2).float()], 2).cuda()
    segs = torch.zeros(G, 224, 224, device="cuda")
    th = torch.from_numpy(synthetic.make_thetas(G * STAGES, seed=9)).cuda()
    real = mocap_real(engine, th[:, 3:75].contiguous(), th[:, 75:].contiguous())
    N = G * STAGES
    drops = [((torch.rand(2, G, 1024, generator=g) >= 0.5).float() * 2.0).cuda() for _ in range(STEPS)]
    interps = [tuple(torch.rand(s, generator=g).cuda() for s in ((N, 14, 3), (N, 10), (N, 24, 3, 3))) for _ in range(STEPS)]
    return images, segs, kp, real, drops, interps


def rows_of(rank, world):
    """this rank's rows of the batch and of the stage-major G * STAGES rows"""
    lo, hi = hpe_amd.distributed.shard_bounds(G, rank, world)
    return slice(lo, hi), [s * G + b for s in range(STAGES) for b in range(lo, hi)]


def run_steps(tr, inputs, rank=0, world=1, after_step=None):
    images, segs, kp, real, drops, interps = inputs
    b, n = rows_of(rank, world)
    c = lambda t: t.contiguous()  # noqa: E731
    out = []
    for i in range(STEPS):
        r = tr.train_step(c(images[b]), c(segs[b]), c(kp[b]), *(c(t[n]) for t in real), drop=c(drops[i][:, b]), interp=tuple(c(t[n]) for t in interps[i]))
        out.append({"losses": [float(x) for x in r["kpr_losses"] + r["generator_critic_losses"]] + [float(r["critic_network_loss"]), float(r["critic_penalty"])],
                    "thetas": [t.cpu() for t in r["thetas"]]})
        if after_step is not None:
            after_step(i)
    return out


def tensors_of(tr):
    g = tr.generator
    return [g.params.detach(), g.encoder_params.detach(), tr.critic.params.detach(), g.encoder_stats]


def world1(port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HPE_FORCE_DIST="1")
    torch.cuda.set_device(0)
    tr = make_trainer()
    assert tr.reducer is None
    inputs = make_inputs(tr.engine)
    plain = run_steps(tr, inputs)
    plain_t = [t.cpu().clone() for t in tensors_of(tr)]
    tr.engine.close()
    torch.distributed.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    n_ar = [0]
    real_ar = torch.distributed.all_reduce

    def counting(*a, **k):
        n_ar[0] += 1
        return real_ar(*a, **k)

    torch.distributed.all_reduce = counting
    tr = make_trainer()
    red = tr.reducer
    assert red is not None and red.active and (red.rank, red.world, red.backend) == (0, 1, "nccl")
    assert red.counts["broadcast"] >= 4 and n_ar[0] == 0  # the replicas start from rank 0's tensors
    per_step = []

    def after(i):
        per_step.append((n_ar[0], dict(red.counts)))

    grouped = run_steps(tr, inputs, after_step=after)
    torch.cuda.synchronize()
    # per step: the hook on every layer's sums, 3 packed blocks (the visible count, the generator's losses, the critic's sums), 3 flat gradients
    for i, (ar, counts) in enumerate(per_step):
        assert ar == (i + 1) * (HOOKS_PER_STEP + 3 + 3), (i, ar)
        assert (counts["hook"], counts["block"], counts["grad"]) == ((i + 1) * HOOKS_PER_STEP, (i + 1) * 3, (i + 1) * 3), counts
    for a, b in zip(plain, grouped):
        assert a["losses"] == b["losses"], (a["losses"], b["losses"])
        assert all(torch.equal(x, y) for x, y in zip(a["thetas"], b["thetas"]))
    for a, b in zip(plain_t, tensors_of(tr)):
        assert torch.equal(a, b.cpu())
    torch.distributed.destroy_process_group()
    open(out_path, "w").write("DP_WORLD1_OK all_reduce per step %d\n" % (HOOKS_PER_STEP + 6))
    print("DP_WORLD1_OK")


def world2(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
    torch.cuda.set_device(0)
    hpe_amd.distributed.Reducer.from_env(backend="gloo", timeout_s=120.0)  # a finite timeout: a rank that dies fails the other
    tr = make_trainer()
    red = tr.reducer
    assert red is not None and (red.rank, red.world, red.backend) == (rank, 2, "gloo") and tr.local_batch == 1
    inputs = make_inputs(tr.engine)
    sums = []

    def after(i):
        torch.cuda.synchronize()
        mine = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in tensors_of(tr)]
        both = [None, None]
        torch.distributed.all_gather_object(both, mine)
        assert both[0] == both[1], "the replicas drifted at step %d" % (i + 1)
        sums.append(mine)

    out = run_steps(tr, inputs, rank, 2, after_step=after)
    assert sums[0] != sums[1]  # the step moved them
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), losses=np.asarray(out[0]["losses"], np.float64),
             thetas=np.stack([t.numpy() for t in out[0]["thetas"]]))
    if rank == 0:
        images, segs, kp, real, drops, interps = inputs
        np.savez(os.path.join(out_dir, "inputs.npz"), kp=kp.cpu().numpy(), **{"real%d" % i: t.cpu().numpy() for i, t in enumerate(real)},
                 **{"interp%d" % i: t.cpu().numpy() for i, t in enumerate(interps[0])})
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
    print("DP_WORLD2_OK rank %d" % rank)


if __name__ == "__main__":
    if sys.argv[1] == "world1":
        world1(sys.argv[2], sys.argv[3])
    else:
        world2(int(sys.argv[2]), sys.argv[3], sys.argv[4])
