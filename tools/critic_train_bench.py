"""hpe_critic_weight_grad and the whole CriticTrainer.step timed against their yardsticks on the same GPU, in the same process: the
forward + input gradient on the same rows (hpe_critic + hpe_critic_backward), and the fp32 torch restatement of the critic update
(tests/critic_train_ref.py: autograd with create_graph=True double backward + torch Adam on the 18 tensors) -- what a user without the
HIP weight gradient would run.  Prints one JSON line and a table; sets no gate.

The method of tools/critic_bench.py: every shape is warmed up, each window is `--iters` calls between two device events (median of
`--repeats` windows, the variants alternated inside each repeat), no profiler attached.  The HIP rows go through HpeEngine, output
allocation included, as the torch rows include theirs.

    python tools/critic_train_bench.py [--iters N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

import hpe_amd
from hpe_amd import synthetic
import critic_train_ref as T
from critic_bench import measure

SHAPES = {"kcs": (13, 13), "joints": (14, 3), "betas": (10,), "Rs": (23, 3, 3)}


def make_rows(eng, N, seed):
    theta = torch.from_numpy(synthetic.make_thetas(N, seed=seed)).cuda()
    outs = [eng.smpl(theta[lo : lo + 256], want=("joints", "Rs")) for lo in range(0, N, 256)]
    return torch.cat([o["joints"] for o in outs])[:, :14].contiguous(), theta[:, 75:].contiguous(), torch.cat([o["Rs"] for o in outs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    params = synthetic.make_critic_params()
    eng = hpe_amd.HpeEngine(device=0, max_batch=256)
    eng.load_smpl(synthetic.make_smpl_model())
    eng.load_critic(params)
    eng.finalize()
    rows = []
    for N in (1, 64, 256, 768, 2304):
        joints, betas, Rs = make_rows(eng, N, seed=N)
        g = torch.Generator().manual_seed(N)
        gs = torch.randn((N, 3), generator=g).cuda()
        tg = {k: torch.randn(s, generator=g).cuda() for k, s in SHAPES.items()}
        eng.critic_reserve(N)

        def fwd_bwd():
            eng.critic(joints, betas, Rs)
            eng.critic_backward(joints, betas, Rs, gs, want=("kcs", "joints", "betas", "Rs"))

        row = {"N": N}
        row.update(measure({"first_order_ms": lambda: eng.critic_weight_grad(joints, betas, Rs, grad_scores=gs),
                            "tangent_ms": lambda: eng.critic_weight_grad(joints, betas, Rs, tangents=tg),
                            "both_ms": lambda: eng.critic_weight_grad(joints, betas, Rs, grad_scores=gs, tangents=tg),
                            "critic_forward_backward_ms": fwd_bwd}, args.iters, args.repeats))
        rows.append(row)
    res = {"tool": "critic_train_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats,
           "weight_grad": rows}
    # the whole critic step at 256 x 3 real and fake rows
    N = 768
    real, fake = make_rows(eng, N, seed=1), make_rows(eng, N, seed=2)
    trainer = hpe_amd.CriticTrainer(eng, generator=torch.Generator(device="cuda").manual_seed(3))
    net = T.net_with_weight_grad(params, torch.float32, "cuda")
    opt = torch.optim.Adam(list(net.P.values()), lr=hpe_amd.critic_train.CRITIC_LR, eps=hpe_amd.critic_train.ADAM_EPS)
    gen = torch.Generator(device="cuda").manual_seed(4)

    def torch_step():
        interp = tuple(torch.rand(t.shape, generator=gen, device="cuda") for t in fake)
        opt.zero_grad(set_to_none=True)
        T.wgan_loss(net, real, fake, interp)["loss"].backward()
        opt.step()

    def hip_inputs_only():  # the yardstick inside the step: scores of real and fake, input gradient at the interpolated rows
        eng.critic(real[0], real[1], real[2])
        eng.critic(fake[0], fake[1], fake[2])
        eng.critic_backward(fake[0], fake[1], fake[2], None, want=("kcs", "joints", "betas", "Rs"))

    res["step_N768"] = measure({"hip_step_ms": lambda: trainer.step(real, fake), "torch_step_ms": torch_step,
                                "hip_loss_only_ms": lambda: hpe_amd.critic_wgan_loss(eng, real, fake, return_grad=False, generator=trainer.generator),
                                "hip_forward_backward_ms": hip_inputs_only}, max(1, args.iters // 4), args.repeats)
    line = json.dumps(res)
    print(line)
    print("%5s %12s %10s %10s %16s" % ("N", "first-order", "tangent", "both", "critic fwd+bwd"))
    for r in rows:
        print("%5d %12.4f %10.4f %10.4f %16.4f" % (r["N"], r["first_order_ms"], r["tangent_ms"], r["both_ms"], r["critic_forward_backward_ms"]))
    s = res["step_N768"]
    print("critic step, 768 real + 768 fake rows: HIP %.3f ms, fp32 torch restatement %.3f ms; loss only %.3f ms; "
          "hpe_critic x2 + hpe_critic_backward %.3f ms" % (s["hip_step_ms"], s["torch_step_ms"], s["hip_loss_only_ms"], s["hip_forward_backward_ms"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
