"""Where the time of encoding a batch of frames as JPEG streams goes: B = 64 RGB frames of 200 x 300 at 4:2:0 and the defaults
(quality 95), the size of LSP's frames.  Rows: the one launch (hpe_jpeg_forward) by device events, the device-to-host copy of the
coefficients into pinned memory, the host entropy pass on 1, 8 and 16 threads, and the whole ``encode_jpeg_batch`` as wall time to
bytes; beside them Pillow's encode of the same frames on 1 and 8 threads plus the device-to-host copy of the pixels it would need --
the yardstick, since there was no JPEG encoder here before.  Prints one JSON line and writes profiles/jpeg_encode_bench.json.

    python tools/jpeg_encode_bench.py [--iters 10] [--out profiles/jpeg_encode_bench.json]

Timing as tools/png_bench.py: host passes are wall time, median of 5 runs after one warm-up; device work is device events around
`iters` back-to-back calls after 3 warm-up calls, median of 5 such groups.  The frames are smooth ramps plus noise of sigma 12, so the
streams have the size of photographs'.  No speed is promised: the coefficients coming down (3 bytes per pixel at 4:2:0) are as large as
the pixels, so the device saves the arithmetic, not the transfer."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import _lib, batch_io, jpeg_encode  # noqa: E402

B, H, W = 64, 200, 300


def wall_ms(fn, runs=5):
    fn()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def event_ms(fn, iters):
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


def frames_host():
    rng = np.random.RandomState(5)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for b in range(B):
        ramp = np.stack([255 * xx / (W - 1), 255 * yy / (H - 1), 255 * ((xx + yy + 7 * b) % (H + W)) / (H + W)], axis=2)
        out.append(np.clip(ramp + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_bench.json"))
    args = ap.parse_args()
    host = frames_host()
    frames = torch.from_numpy(host).cuda()
    lib = _lib.load()
    res = {"batch": B, "height": H, "width": W, "subsampling": "4:2:0", "quality": 95, "pixel_bytes": int(host.nbytes)}

    buf, shapes, offsets = batch_io.pack_frames(frames, jpeg_encode.CHANNELS)
    table, totals = jpeg_encode.encode_layout(shapes, offsets, 95, "4:2:0")
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    coef = torch.empty(int(totals[0]), dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def launch():
        _lib.check(lib.hpe_jpeg_forward(p(table), table_dev.data_ptr(), B, buf.data_ptr(), buf.numel(), coef.data_ptr(), coef.numel(), st))

    res["coef_bytes"] = int(coef.numel() * 2)
    res["workgroups"] = int(totals[1])
    res["forward_launch_ms"] = event_ms(launch, args.iters)
    pinned = torch.empty(coef.numel(), dtype=torch.int16, pin_memory=True)
    res["d2h_coef_ms"] = event_ms(lambda: pinned.copy_(coef, non_blocking=True), args.iters)
    torch.cuda.synchronize()
    coef_host = pinned.numpy().copy()
    out = np.empty(int(totals[2]), np.uint8)
    streams = None
    for t in (1, 8, 16):
        res["host_entropy_ms_threads%d" % t] = wall_ms(lambda: jpeg_encode.entropy_encode(coef_host, table, threads=t, out=out))
    streams = jpeg_encode.entropy_encode(coef_host, table, threads=8, out=out)
    res["stream_bytes_mean"] = float(np.mean([len(s) for s in streams]))
    res["encode_jpeg_batch_wall_ms"] = wall_ms(lambda: hpe_amd.encode_jpeg_batch(frames))
    res["encode_jpeg_batch_wall_ms_threads16"] = wall_ms(lambda: hpe_amd.encode_jpeg_batch(frames, threads=16))

    pix = torch.empty(frames.numel(), dtype=torch.uint8, pin_memory=True)
    res["d2h_pixels_ms"] = event_ms(lambda: pix.copy_(frames.reshape(-1), non_blocking=True), args.iters)
    torch.cuda.synchronize()
    try:
        from PIL import Image

        def one(f):
            b = io.BytesIO()
            Image.fromarray(f).save(b, "JPEG", quality=95, subsampling="4:2:0", dpi=(300, 300))
            return b.getvalue()

        res["equals_pillow"] = [one(f) for f in host] == streams
        res["pillow_encode_ms_threads1"] = wall_ms(lambda: [one(f) for f in host])
        with ThreadPoolExecutor(max_workers=8) as pool:
            res["pillow_encode_ms_threads8"] = wall_ms(lambda: list(pool.map(one, host)))
        for t in (1, 8):
            res["pillow_d2h_and_encode_ms_threads%d" % t] = res["d2h_pixels_ms"] + res["pillow_encode_ms_threads%d" % t]
        res["encode_jpeg_batch_over_pillow_and_d2h_threads8"] = res["encode_jpeg_batch_wall_ms"] / res["pillow_d2h_and_encode_ms_threads8"]
    except ImportError:
        res["equals_pillow"] = None
    res["not_measured"] = ["power", "frames larger than 200 x 300", "4:4:4 and 4:2:2", "several GPUs", "the launch under a concurrent training step"]
    line = json.dumps({"frames_200x300_rgb_b64_q95_420": res})
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
