"""ms per hpe_encoder_backward, per hpe_encoder_set_params (host) and per hpe_encoder_set_params_dev (device) at B in {8, 32, 64}, against the same ResNet-50 (frozen BatchNorm statistics)
in torch fp32 with autograd in the same process.  Prints one JSON line and writes profiles/encoder_train_bench.json.

    python tools/encoder_train_bench.py [--batches 8,32,64] [--iters 10] [--out profiles/encoder_train_bench.json]

Timing: device events around `iters` back-to-back calls after 3 warm-up calls, median of 5 such groups (the backward, torch and the device
update alike; the host update is wall time over 3 calls); torch's TF32 paths are off.  `set_params_dev_bytes_written` is what one device
update writes at the default plan (every packing the context holds, from hpe_debug_encoder_packing_bytes), `set_params_dev_write_GBps`
those bytes over the measured time.

    python tools/encoder_train_bench.py --bn batch [--out profiles/encoder_bn_train_bench.json]

The batch-statistics leg, same method: ms per hpe_encoder_backward_batchnorm, per frozen hpe_encoder_backward in the same run, per
hpe_encoder_update_stats + hpe_encoder_set_stats_dev, against torch fp32 autograd of the same ResNet-50 with F.batch_norm(training=True).

    python tools/encoder_train_bench.py --precision bf16 [--out profiles/encoder_train_mixed_bench.json]

The mixed-precision leg: ms per hpe_encoder_backward_mixed and per fp32 hpe_encoder_backward on the same context, the two alternating group
by group (same events, 5 groups of `iters` calls each after 3 warm-up calls of each, medians), and the bytes of the two reserves.

    python tools/encoder_train_bench.py --bn batch --precision mixed [--out profiles/encoder_bn_mixed_bench.json]

The mixed-precision leg with batch statistics, same method: ms per hpe_encoder_backward_batchnorm_mixed and per fp32
hpe_encoder_backward_batchnorm on the same context, alternating group by group, and the bytes of the reserves."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import _lib, synthetic  # noqa: E402
from hpe_amd.resnet_spec import CONV_SPECS, STAGE_BLOCKS  # noqa: E402


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


def timed_pair(fn_a, fn_b, iters):
    """timed() for two calls that alternate group by group, so that both see the same clocks and the same neighbours"""
    for _ in range(3):
        fn_a()
        fn_b()
    groups = ([], [])
    for _ in range(5):
        for fn, out in ((fn_a, groups[0]), (fn_b, groups[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) / iters)
    return statistics.median(groups[0]), statistics.median(groups[1])


class TorchResNet(object):
    """the same function in torch: NCHW conv2d + the folded affine of the fixed statistics + ReLU; gradients to W, b, gamma, beta"""

    def __init__(self, params, eps=1e-3, batch_norm=False):
        self.layers, self.eps, self.batch_norm = [], eps, batch_norm
        for s in CONV_SPECS:
            t = lambda k: torch.from_numpy(np.asarray(params[k], np.float32)).cuda()  # noqa: E731
            W = t(s.name + "/kernel").permute(3, 2, 0, 1).contiguous().requires_grad_(True)
            b, gamma, beta = (t(k).requires_grad_(True) for k in (s.name + "/bias", s.bn_name + "/gamma", s.bn_name + "/beta"))
            mean, istd = t(s.bn_name + "/moving_mean"), 1.0 / torch.sqrt(t(s.bn_name + "/moving_variance") + eps)
            self.layers.append((s, W, b, gamma, beta, mean, istd))
        self.leaves = [p for l in self.layers for p in l[1:5]]

    def conv(self, i, x, res=None, relu=True):
        s, W, b, gamma, beta, mean, istd = self.layers[i]
        if self.batch_norm:  # BatchNorm in training mode: the statistics of the batch, the gradient through them
            z = F.conv2d(x, W, bias=b, stride=s.stride, padding=(s.kh - 1) // 2)
            y = F.batch_norm(z, None, None, gamma, beta, training=True, eps=self.eps)
            if res is not None:
                y = y + res
            return torch.relu(y) if relu else y
        z = F.conv2d(x, W, stride=s.stride, padding=(s.kh - 1) // 2)
        y = (gamma * istd).view(1, -1, 1, 1) * (z + (b - mean).view(1, -1, 1, 1)) + beta.view(1, -1, 1, 1)
        if res is not None:
            y = y + res
        return torch.relu(y) if relu else y

    def features(self, img):
        x = self.conv(0, img.permute(0, 3, 1, 2))
        x = F.max_pool2d(F.pad(x, (1, 1, 1, 1)), 3, 2)
        ci = 1
        for stage in (2, 3, 4, 5):
            for b in range(STAGE_BLOCKS[stage]):
                t = self.conv(ci + 1, self.conv(ci, x))
                res = self.conv(ci + 3, x, relu=False) if b == 0 else x
                x = self.conv(ci + 2, t, res)
                ci += 4 if b == 0 else 3
        return x.mean((2, 3))

    def backward(self, img, gf):
        for p in self.leaves:
            p.grad = None
        (self.features(img) * gf).sum().backward()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="8,32,64")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bn", choices=("frozen", "batch"), default="frozen")
    ap.add_argument("--precision", choices=("fp32", "bf16", "mixed"), default="fp32",
                    help="bf16: the mixed-precision leg (frozen statistics only); mixed: the same, or with --bn batch the mixed-precision leg with batch statistics")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-calls", type=int, default=0,
                    help="run only this many backward calls of the chosen mode at the first batch and exit: the workload of a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    bn, mixed = a.bn == "batch", a.precision != "fp32"
    if bn and a.precision == "bf16":
        ap.error("--precision bf16 runs with frozen statistics only: --precision mixed takes --bn batch")
    if a.out is None:
        name = ("encoder_bn_mixed_bench.json" if bn else "encoder_train_mixed_bench.json") if mixed else "encoder_bn_train_bench.json" if bn else "encoder_train_bench.json"
        a.out = os.path.join(ROOT, "profiles", name)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    batches = [int(b) for b in a.batches.split(",")]
    params = synthetic.make_encoder_params()
    eng = hpe_amd.HpeEngine(device=0, max_batch=max(batches))
    eng.load_encoder(params)
    eng.finalize()
    eng.reserve_encoder_train(max(batches), batch_norm=bn, precision=a.precision)
    if a.trace_calls:
        img = torch.from_numpy(synthetic.make_images(batches[0], seed=1)).cuda()
        gf = torch.randn(batches[0], 2048, device="cuda")
        for _ in range(a.trace_calls):
            eng.encoder_backward(img, gf, bn=a.bn, precision=a.precision)
        torch.cuda.synchronize()
        eng.close()
        return
    if mixed:
        res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "method": "device events, the two calls alternating, median of 5 groups after 3 warm-ups",
               "rows": []}
        for B in batches:
            img = torch.from_numpy(synthetic.make_images(B, seed=1)).cuda()
            gf = torch.randn(B, 2048, device="cuda")
            mx, f32 = timed_pair(lambda: eng.encoder_backward(img, gf, bn=a.bn, precision=a.precision), lambda: eng.encoder_backward(img, gf, bn=a.bn),
                                 a.iters)
            if bn:
                res["rows"].append({"B": B, "hpe_encoder_backward_batchnorm_mixed_ms": round(mx, 3), "hpe_encoder_backward_batchnorm_ms": round(f32, 3),
                                    "fp32_over_mixed": round(f32 / mx, 3),
                                    "reserve_fp32_batchnorm_bytes": 4 * eng.lib.hpe_encoder_train_ws_floats_batchnorm(B),
                                    "reserve_batchnorm_mixed_bytes": 4 * eng.lib.hpe_encoder_train_ws_floats_batchnorm_mixed(B)})
                continue
            res["rows"].append({"B": B, "hpe_encoder_backward_mixed_ms": round(mx, 3), "hpe_encoder_backward_ms": round(f32, 3),
                                "fp32_over_mixed": round(f32 / mx, 3), "reserve_fp32_bytes": 4 * eng.lib.hpe_encoder_train_ws_floats(B),
                                "reserve_fp32_and_mixed_bytes": 4 * eng.lib.hpe_encoder_train_ws_floats_mixed(B)})
        eng.close()
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
        return
    ref = TorchResNet(params, batch_norm=bn)
    flat_dev = eng.encoder_params()
    flat = flat_dev.cpu()
    written = sum(eng.lib.hpe_debug_encoder_packing_bytes(eng._h, i, w) for i in range(len(CONV_SPECS)) for w in range(len(_lib.ENCODER_PACKINGS)))
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "set_params_dev_bytes_written": written, "rows": []}
    for B in batches:
        img = torch.from_numpy(synthetic.make_images(B, seed=1)).cuda()
        gf = torch.randn(B, 2048, device="cuda")
        if bn:
            stats = eng.encoder_stats()
            hip = timed(lambda: eng.encoder_backward(img, gf, bn="batch"), a.iters)
            frozen = timed(lambda: eng.encoder_backward(img, gf), a.iters)
            tch = timed(lambda: ref.backward(img, gf), a.iters)
            upd = timed(lambda: eng.set_encoder_stats_dev(eng.update_encoder_stats(stats, 1.0)), a.iters)  # momentum 1: the statistics stay
            res["rows"].append({"B": B, "hpe_encoder_backward_batchnorm_ms": round(hip, 3), "hpe_encoder_backward_ms": round(frozen, 3),
                                "torch_autograd_batchnorm_fwd_bwd_ms": round(tch, 3), "update_and_set_stats_dev_ms": round(upd, 3)})
            continue
        hip = timed(lambda: eng.encoder_backward(img, gf), a.iters)
        tch = timed(lambda: ref.backward(img, gf), a.iters)
        t0 = time.perf_counter()
        for _ in range(3):
            eng.set_encoder_params(flat)
        setp = (time.perf_counter() - t0) / 3 * 1e3
        setd = timed(lambda: eng.set_encoder_params_dev(flat_dev), a.iters)
        res["rows"].append({"B": B, "hpe_encoder_backward_ms": round(hip, 3), "torch_autograd_fwd_bwd_ms": round(tch, 3),
                            "hpe_encoder_set_params_ms": round(setp, 1), "hpe_encoder_set_params_dev_ms": round(setd, 3),
                            "set_params_dev_write_GBps": round(written / setd / 1e6, 1)})
    eng.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
