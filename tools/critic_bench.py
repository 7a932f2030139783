"""hpe_critic / hpe_critic_backward timing against the fp32 torch restatement of the critic (tests/critic_ref.py) on the same GPU, in
the same process: what a user without the HIP critic would run.  Also the cost the critic term adds to Predictor.val_step at B = 256.
Prints one JSON line and a table; sets no gate.

N in {1, 64, 256, 768} (768 = B 256 x three stages).  Every shape is warmed up, each window is `--iters` calls between two device
events (median of `--repeats` windows, the variants alternated inside each repeat), no profiler attached.  The HIP rows go through
HpeEngine.critic / critic_backward, output allocation included, as the torch rows include theirs.

    python tools/critic_bench.py [--iters N] [--repeats R] [--no-val-step] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import hpe_amd
from hpe_amd import synthetic
from critic_ref import CriticTorch


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(fns, iters, repeats):
    for fn in fns.values():  # warm-up of every shape
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            samples[k].append(window(fn, iters))
    row = {}
    for k, v in samples.items():
        row[k] = round(statistics.median(v), 4)
        row[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-val-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    model = synthetic.make_smpl_model()
    params = synthetic.make_critic_params()
    eng = hpe_amd.HpeEngine(device=0, max_batch=256)
    eng.load_smpl(model)
    eng.load_critic(params)
    eng.finalize()
    ref = CriticTorch(params, torch.float32, device="cuda")
    rows = []
    for N in (1, 64, 256, 768):
        theta = torch.from_numpy(synthetic.make_thetas(N, seed=N)).cuda()
        outs = [eng.smpl(theta[lo : lo + 256], want=("joints", "Rs")) for lo in range(0, N, 256)]
        joints, Rs = torch.cat([o["joints"] for o in outs]), torch.cat([o["Rs"] for o in outs])
        betas = theta[:, 75:]
        gs = torch.randn((N, 3), generator=torch.Generator().manual_seed(N)).cuda()

        def hip_fwd_bwd():
            eng.critic(joints, betas, Rs)
            eng.critic_backward(joints, betas, Rs, gs)

        def torch_fwd():
            with torch.no_grad():
                ref(joints, betas, Rs)

        def torch_fwd_bwd():
            j, b, r = joints.clone().requires_grad_(True), betas.clone().requires_grad_(True), Rs.clone().requires_grad_(True)
            torch.autograd.grad(ref(j, b, r), [j, b, r], gs)

        row = {"N": N}
        row.update(measure({"hip_forward_ms": lambda: eng.critic(joints, betas, Rs), "hip_forward_backward_ms": hip_fwd_bwd,
                            "torch_forward_ms": torch_fwd, "torch_forward_backward_ms": torch_fwd_bwd}, args.iters, args.repeats))
        rows.append(row)
    res = {"tool": "critic_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": rows}
    if not args.no_val_step:
        B = 256

        class Cfg(object):
            img_size, num_stage, batch_size, data_format = 224, 3, B, "NHWC"
            checkpoint_dir = smpl_model_path = None

        p = hpe_amd.Predictor(Cfg(), smpl_model=model, mean_params=synthetic.make_mean_params(), encoder_params=synthetic.make_encoder_params(),
                              regressor_params=synthetic.make_regressor_params(variant="bounded"), critic_params=params)
        img = torch.from_numpy(synthetic.make_images(B, seed=1)).cuda()
        seg, kp = synthetic.make_lsp_targets(B, seed=2)
        seg, kp = torch.from_numpy(seg).cuda(), torch.from_numpy(kp).cuda()
        res["val_step_B256"] = measure({"without_critic_ms": lambda: p.val_step(img, seg, kp),
                                        "with_critic_ms": lambda: p.val_step(img, seg, kp, critic_loss_weight=0.01)},
                                       max(1, args.iters // 20), args.repeats)
    line = json.dumps(res)
    print(line)
    print("%4s %10s %12s %11s %14s" % ("N", "hip fwd", "hip fwd+bwd", "torch fwd", "torch fwd+bwd"))
    for r in rows:
        print("%4d %10.4f %12.4f %11.4f %14.4f" % (r["N"], r["hip_forward_ms"], r["hip_forward_backward_ms"], r["torch_forward_ms"],
                                                   r["torch_forward_backward_ms"]))
    if "val_step_B256" in res:
        print("val_step B=256: %.3f ms without the critic term, %.3f ms with it" % (res["val_step_B256"]["without_critic_ms"],
                                                                                   res["val_step_B256"]["with_critic_ms"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
