"""ms per KerasAdam.step with and without the guard (global-norm clipping, skip on a non-finite gradient; csrc/adam.hip) at the sizes
of the real updates: the generator's (the encoder's flat tensor and the regressor's under one optimiser) and the critic's.  Per update:
the unguarded step, the guarded step with one segment per tensor, the guarded step with the per-layer tables the trainers register
(optim.layer_segments), and hpe_grad_stats alone with its achieved bytes/s (4 bytes per element, read once).  Prints one JSON line and
writes profiles/grad_guard_bench.json.

    python tools/grad_guard_bench.py [--iters 10] [--out profiles/grad_guard_bench.json]
    python tools/grad_guard_bench.py --lib /path/to/another/libhpe_hip.so     # the unguarded step alone on another build (a baseline)

Timing: device events around `iters` back-to-back calls after 3 warm-up calls, median of 5 such groups (tools/adam_bench.py's method);
gradients fixed and finite, clipping active (global_clipnorm = 1), so every guarded step multiplies and stores."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import _lib  # noqa: E402

GUARD_ENTRY_POINTS = ("hpe_grad_stats_chunk", "hpe_grad_stats_workspace_bytes", "hpe_grad_stats", "hpe_adam_guard", "hpe_adam_apply_guarded")


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


def optimiser(sizes, tables=None, **kw):
    g = torch.Generator(device="cuda").manual_seed(1)
    opt = hpe_amd.KerasAdam(1e-4, 0.9, 0.999, 1e-7, **kw)
    for name, n in sizes:
        p = opt.add(name, torch.randn(n, generator=g, device="cuda"), **({"segments": tables[name]} if tables else {}))
        p.grad = torch.randn(n, generator=g, device="cuda") * 1e-2
    return opt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_guard_bench.json"))
    a = ap.parse_args()
    if a.lib:  # another build: bind what it has of the guard's entry points (a build from before them has none)
        assert _lib._lib is None, "the library is loaded already"
        _lib.LIB_PATH = os.path.abspath(a.lib)
        probe = C.CDLL(_lib.LIB_PATH, mode=C.RTLD_GLOBAL)
        for name in GUARD_ENTRY_POINTS:
            if not hasattr(probe, name):
                _lib._PROTOS.pop(name)
    lib = _lib.load()
    from hpe_amd.optim import layer_segments

    updates = {"generator": (("encoder", lib.hpe_encoder_param_floats()), ("regressor", lib.hpe_regressor_param_floats())),
               "critic": (("critic", lib.hpe_critic_param_floats()),)}
    rows = []
    for update, sizes in updates.items():
        n = sum(k for _name, k in sizes)
        row = {"update": update, "floats": n, "unguarded_step_ms": round(timed(optimiser(sizes).step, a.iters), 4)}
        if not a.lib:
            tables = {name: layer_segments(name, lib)[0] for name, _k in sizes}
            one, per_layer = optimiser(sizes, global_clipnorm=1.0, skip_nonfinite=True), optimiser(sizes, tables, global_clipnorm=1.0, skip_nonfinite=True)
            # alternate the three, so that a drift of the clock shows in all of them
            row["unguarded_step_ms_again"] = round(timed(optimiser(sizes).step, a.iters), 4)
            row["guarded_step_ms"] = round(timed(one.step, a.iters), 4)
            row["guarded_step_per_layer_ms"] = round(timed(per_layer.step, a.iters), 4)
            row["segments_per_layer"] = sum(len(t) - 1 for t in tables.values())
            assert one.clipped_steps == per_layer.clipped_steps == 3 + 5 * a.iters and one.skipped_steps == 0
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for label, opt in (("grad_stats", one), ("grad_stats_per_layer", per_layer)):
                def stats(opt=opt):
                    for name, p in opt.params.items():
                        off_dev, rec, ws, nbytes = opt._stats[name]
                        off = opt.segments[name]
                        _lib.check(lib.hpe_grad_stats(p.grad.data_ptr(), p.numel(), off.ctypes.data, off_dev.data_ptr(), off.size - 1, rec.data_ptr(),
                                                      ws.data_ptr(), nbytes, stream))
                ms = timed(stats, a.iters)
                row[label + "_ms"], row[label + "_TBps"] = round(ms, 4), round(4 * n / (ms * 1e-3) / 1e12, 3)
            row["bytes_unguarded"], row["bytes_guarded"] = 28 * n, 32 * n
        rows.append(row)
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "library": a.lib or "this build", "rows": rows}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
