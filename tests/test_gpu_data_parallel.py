"""hpe_amd.Trainer under a process group, in fresh child processes (tests/_dp_trainer_worker.py): a world of one over ``nccl`` with
HPE_FORCE_DIST=1 against the same steps without a group, bit for bit; and two ``gloo`` ranks on the one GPU, whose replicas must never
drift and whose reported losses are those of the global batch.

The losses of the world-2 run are compared with the float64 restatement of the SAME G = 2 batch on the CPU (tests/smpl_torch_ref.py,
tests/critic_ref.py, tests/critic_train_ref.py, tests/regressor_train_ref.py's kp_loss), computed from the ranks' gathered thetas of
step 1 -- taken before any update.  The bar is the project's: 4 x the error of the same restatement in float32, here the worst relative
error over the eight reported losses on both sides.  Parameters after the update are not compared with a single-process run: Adam's
first step is +-lr, which turns a last-bit difference of a gradient into 2 * lr.

Figures of one run on an MI355X: DESIGN.md "Data-parallel training"."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import critic_ref
import critic_train_ref as CT
import regressor_train_ref as RR
from hpe_amd import synthetic
from smpl_torch_ref import SmplTorch

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dp_trainer_worker.py")
MARGIN = 4.0
G, STAGES = 2, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return str(p)


def test_world_of_one_over_nccl_is_bit_exact(tmp_path):
    """two train_steps at B = 2 with fixed drop / interp: losses, thetas and the flat tensors have the bits of the run without a group;
    159 hook calls, 3 packed blocks and 3 flat gradients per step, each one all-reduce"""
    out = tmp_path / "world1.txt"
    r = subprocess.run([sys.executable, WORKER, "world1", _free_port(), str(out)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "DP_WORLD1_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert out.read_text().startswith("DP_WORLD1_OK")


def _restated_losses(thetas, inp, dtype):
    """the eight losses train_step reports -- 60 x kp and 0.01 x critic term of every stage, the critic's loss and its penalty -- of the
    global batch, from the stages' thetas [S,G,85]"""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    smpl = SmplTorch(synthetic.make_smpl_model(), dtype)
    critic = critic_ref.CriticTorch(synthetic.make_critic_params(), dtype)
    kp_gt = t(inp["kp"])
    outs = [smpl(t(th)) for th in thetas]
    kpr = [60.0 * RR.kp_loss(kp_gt, o["kp2d"]) for o in outs]
    gc = [0.01 * -critic(o["joints"], t(th)[:, 75:], o["Rs"]).mean(0).sum() for o, th in zip(outs, thetas)]
    fake = (torch.cat([o["joints"] for o in outs]), torch.cat([t(th)[:, 75:] for th in thetas]), torch.cat([o["Rs"] for o in outs]))
    real = tuple(t(inp["real%d" % i]) for i in range(3))
    interp = tuple(t(inp["interp%d" % i]) for i in range(3))
    w = CT.wgan_loss(critic, real, fake, interp)
    return np.asarray([float(x.detach()) for x in kpr + gc + [w["loss"], w["penalty"]]], np.float64)


def test_two_gloo_ranks_on_one_gpu(tmp_path):
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, WORKER, "world2", str(k), port, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for k in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for k, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and "DP_WORLD2_OK rank %d" % k in o, o[-4000:]
    ranks = [np.load(tmp_path / ("rank%d.npz" % k)) for k in range(2)]
    inp = np.load(tmp_path / "inputs.npz")
    # every rank reports the losses of the GLOBAL batch: the same numbers
    assert np.array_equal(ranks[0]["losses"], ranks[1]["losses"])
    thetas = np.concatenate([r["thetas"] for r in ranks], 1)  # [S, G, 85], rank order = row order
    assert thetas.shape == (STAGES, G, 85)
    ref = _restated_losses(thetas, inp, torch.float64)
    f32 = _restated_losses(thetas, inp, torch.float32)
    err = lambda a: float(np.max(np.abs(a - ref) / np.abs(ref)))  # noqa: E731
    e, bar = err(ranks[0]["losses"]), MARGIN * err(f32)
    print("world-2 gloo, step 1: reported losses %s\nfloat64 restatement %s\nworst relative error %.3g, bar %.3g (4 x the float32 restatement's)"
          % (ranks[0]["losses"].tolist(), ref.tolist(), e, bar))
    assert e < bar, (e, bar)
