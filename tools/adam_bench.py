"""ms per KerasAdam.step (hpe_adam_advance + hpe_adam_apply, csrc/adam.hip) against torch.optim.Adam.step in the same process, on one flat
float32 tensor of the encoder's size (resnet_spec.encoder_param_count() floats) and of the regressor's (regressor_spec.PARAM_FLOATS).
Prints one JSON line and writes profiles/adam_bench.json.

    python tools/adam_bench.py [--iters 10] [--out profiles/adam_bench.json]

Timing: device events around `iters` back-to-back calls after 3 warm-up calls, median of 5 such groups (tools/encoder_train_bench.py's
method), both optimisers alike, gradients fixed.  `bytes_moved` is what the fused update has to move: p, m, v and g read, p, m and v
written, 28 bytes per element; `TBps` is that over the measured time of each optimiser (torch's own traffic is larger: it runs several
elementwise passes, `torch_foreach` says which implementation torch chose)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import regressor_spec, resnet_spec  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    groups = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        groups.append(a.elapsed_time(b) / iters)
    return statistics.median(groups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.json"))
    a = ap.parse_args()
    rows = []
    for name, n in (("encoder", resnet_spec.encoder_param_count()), ("regressor", regressor_spec.PARAM_FLOATS)):
        g = torch.Generator(device="cuda").manual_seed(1)
        p0 = torch.randn(n, generator=g, device="cuda")
        grad = torch.randn(n, generator=g, device="cuda") * 1e-2
        pk = p0.clone()
        keras = hpe_amd.KerasAdam(1e-4, 0.9, 0.999, 1e-7)
        keras.add(name, pk)
        pk.grad = grad
        pt = p0.clone().requires_grad_(True)
        topt = torch.optim.Adam([pt], lr=1e-4, betas=(0.9, 0.999), eps=1e-7)
        pt.grad = grad.clone()
        k_ms = timed(keras.step, a.iters)
        t_ms = timed(topt.step, a.iters)
        moved = 28 * n
        rows.append({"tensor": name, "floats": n, "bytes_moved": moved, "keras_adam_step_ms": round(k_ms, 4), "torch_adam_step_ms": round(t_ms, 4),
                     "keras_adam_TBps": round(moved / (k_ms * 1e-3) / 1e12, 3), "torch_adam_TBps_same_bytes": round(moved / (t_ms * 1e-3) / 1e12, 3),
                     "torch_foreach": topt.param_groups[0].get("foreach"), "torch_fused": topt.param_groups[0].get("fused")})
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "rows": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
