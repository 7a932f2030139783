"""hpe_smpl / hpe_smpl_backward timing against torch autograd over the torch restatement of the layer (tests/smpl_torch_ref.py),
on the same GPU: what a user without the HIP backward would run.  Prints one JSON line and a table; sets no gate.

B in {1, 64, 256}; cotangent sets: kp2d only, and verts + kp2d.  Every shape is warmed up, each window is `--iters` calls between
two device events (median of `--repeats` windows, the three variants alternated inside each repeat), no profiler attached.  The
torch rows are the restatement's backward alone (its forward graph is built once and kept) and its forward + backward.

    python tools/smpl_backward_bench.py [--iters N] [--repeats R] [--out FILE]
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
from smpl_torch_ref import SmplTorch, make_theta


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device only")
    model = synthetic.make_smpl_model()
    eng = hpe_amd.HpeEngine(device=0, max_batch=256)
    eng.load_smpl(model)
    eng.finalize()
    ref = SmplTorch(model, torch.float32)
    for name in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "kp_regressor"):
        setattr(ref, name, getattr(ref, name).cuda())
    _eye = torch.eye
    rows = []
    for B in (1, 64, 256):
        th = torch.from_numpy(make_theta(B, seed=B)).cuda()
        g = torch.Generator().manual_seed(B)
        cot_all = {"kp2d": torch.randn((B, eng.num_kp, 2), generator=g).cuda(), "verts": torch.randn((B, 6890, 3), generator=g).cuda()}
        for names in (("kp2d",), ("verts", "kp2d")):
            cot = {k: cot_all[k] for k in names}
            x = th.clone().requires_grad_(True)
            torch.eye = lambda *a, **k: _eye(*a, **{**k, "device": "cuda"})  # the restatement builds its identities on the default device
            try:
                out = ref(x)

                def t_bwd():
                    torch.autograd.grad([out[k] for k in names], x, [cot[k] for k in names], retain_graph=True)

                def t_fwd_bwd():
                    o = ref(x)
                    torch.autograd.grad([o[k] for k in names], x, [cot[k] for k in names])

                fns = {
                    "hip_forward_ms": lambda: eng.smpl(th, want=names),
                    "hip_backward_ms": lambda: eng.smpl_backward(th, cot),
                    "torch_backward_ms": t_bwd,
                    "torch_forward_backward_ms": t_fwd_bwd,
                }
                for fn in fns.values():  # warm-up of every shape
                    for _ in range(5):
                        fn()
                torch.cuda.synchronize()
                samples = {k: [] for k in fns}
                for _ in range(args.repeats):
                    for k, fn in fns.items():
                        samples[k].append(window(fn, args.iters))
            finally:
                torch.eye = _eye
            row = {"B": B, "cotangents": "+".join(names)}
            for k, v in samples.items():
                row[k] = round(statistics.median(v), 4)
                row[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
            rows.append(row)
    res = {"tool": "smpl_backward_bench", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "rows": rows}
    line = json.dumps(res)
    print(line)
    print("%4s %-11s %10s %10s %12s %14s" % ("B", "cotangents", "hip fwd", "hip bwd", "torch bwd", "torch fwd+bwd"))
    for r in rows:
        print("%4d %-11s %10.4f %10.4f %12.4f %14.4f" % (r["B"], r["cotangents"], r["hip_forward_ms"], r["hip_backward_ms"], r["torch_backward_ms"],
                                                         r["torch_forward_backward_ms"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
