"""hpe_regressor_backward and the whole GeneratorTrainer.step (from features) timed against their yardstick on the same GPU, in the same
process: the fp32 torch restatement of the same three-stage IEF loop (tests/regressor_train_ref.py: rocBLAS GEMMs, autograd, and
torch Adam on the seven tensors for the step) -- what a user without the HIP backward would run.  Prints one JSON line and a table,
writes profiles/regressor_train_bench.json; sets no gate.

The method of tools/critic_bench.py: every shape is warmed up, each window is `--iters` calls between two device events on the stream
(median of `--repeats` windows, the variants alternated inside each repeat; the spread max - min of the windows is reported beside every
median), no profiler attached.  The HIP rows go through HpeEngine, output allocation included, as the torch rows include theirs.

    python tools/regressor_train_bench.py [--iters N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch

import hpe_amd
from hpe_amd import synthetic
import regressor_train_ref as T
from critic_bench import measure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regressor_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    params, mean = T.fixture_params()
    flat = T.flat_of(params, mean)
    eng = hpe_amd.HpeEngine(device=0, max_batch=256)
    eng.load_smpl(synthetic.make_smpl_model())
    eng.load_regressor(params)
    eng.load_mean_theta(mean)
    eng.load_critic(synthetic.make_critic_params())
    eng.finalize()
    start = eng.regressor_params().clone()
    rows = []
    for B in (1, 8, 64, 256):
        feat = torch.from_numpy(T.make_features(B, seed=B)).cuda()
        drop = torch.from_numpy(T.make_drop(B, seed=B)).cuda()
        gt = torch.randn((T.S, B, 85), generator=torch.Generator().manual_seed(B)).cuda()
        kp_gt = torch.from_numpy(synthetic.make_thetas(B, seed=B)[:, : 19 * 3].reshape(B, 19, 3) * 0.3).cuda().contiguous()
        kp_gt[:, :, 2] = 1.0
        P = T.tensors(flat, torch.float32, "cuda")
        opt = torch.optim.Adam([P[k] for k in T.KEYS], lr=1e-4, eps=1e-7)
        trainer = hpe_amd.GeneratorTrainer(eng, generator=torch.Generator(device="cuda").manual_seed(1))

        def torch_fwd_bwd():
            for p in P.values():
                p.grad = None
            f = feat.clone().requires_grad_(True)
            th, _ = T.ief(P, f, drop)
            (th * gt).sum().backward()

        def torch_step():
            torch_fwd_bwd()
            opt.step()

        def hip_fwd_bwd():
            eng.regressor_forward_train(feat, drop)
            eng.regressor_backward(feat, gt, drop)

        row = {"B": B}
        row.update(measure({"hip_backward_ms": lambda: eng.regressor_backward(feat, gt, drop), "hip_forward_backward_ms": hip_fwd_bwd,
                            "torch_forward_backward_ms": torch_fwd_bwd, "torch_forward_backward_adam_ms": torch_step,
                            "hip_set_params_ms": lambda: eng.set_regressor_params(start),
                            "hip_generator_step_ms": lambda: trainer.step(feat, kp_gt, drop=drop)}, args.iters, args.repeats))
        row["ratio_hip_over_torch"] = round(row["hip_forward_backward_ms"] / row["torch_forward_backward_ms"], 3)
        row["ratio_allowed"] = round(1.0 + row["torch_forward_backward_spread_ms"] / row["torch_forward_backward_ms"], 3)
        eng.set_regressor_params(start)
        rows.append(row)
    res = {"tool": "regressor_train_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": rows}
    line = json.dumps(res)
    print(line)
    print("%5s %12s %14s %16s %18s %10s %12s %8s" % ("B", "hip backward", "hip fwd + bwd", "torch fwd + bwd", "torch fwd+bwd+Adam", "set params",
                                                   "trainer step", "ratio"))
    for r in rows:
        print("%5d %12.4f %14.4f %16.4f %18.4f %10.4f %12.4f %8.3f" % (r["B"], r["hip_backward_ms"], r["hip_forward_backward_ms"],
                                                                      r["torch_forward_backward_ms"], r["torch_forward_backward_adam_ms"],
                                                                      r["hip_set_params_ms"], r["hip_generator_step_ms"], r["ratio_hip_over_torch"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
