"""Where the time of loading one training batch goes: B JPEG streams of about 300 x 200, 4:2:0, through the host entropy pass (1, 8, 16
threads), the one host-to-device copy, the two back-end launches, and the whole ``load_training_batch``.  Where Pillow is importable
its decode of the same streams on the same number of threads plus the upload of the pixels stands beside it: the only comparison with a
meaning, since there was no decoder here before.  Prints one JSON line and writes profiles/jpeg_bench.json.

    python tools/jpeg_bench.py [--batch 64] [--iters 10] [--out profiles/jpeg_bench.json]

Timing: host passes are wall time, median of 5 runs after one warm-up.  Device work is device events around `iters` back-to-back calls
after 3 warm-up calls, median of 5 such groups, as tools/encoder_train_bench.py measures.  The streams are encoded with Pillow when it
is importable (a 200 x 300 ramp plus noise, quality 85); without it the largest fixture (97 x 130) is repeated and the JSON says so."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import _lib, jpeg  # noqa: E402

ENCODER_BACKWARD_B64_MS = 26.74  # hpe_encoder_backward at B = 64, DESIGN.md "Encoder training"


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


def make_streams(B):
    try:
        from PIL import Image
    except ImportError:
        import jpeg_ref as R

        s = R.stream("s420_q30_97x130")
        return [s] * B, [R.stream("seg_40x50")] * 0, "largest fixture (97 x 130) repeated", None
    rng = np.random.RandomState(7)
    H, W = 200, 300
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out, segs = [], []
    for i in range(B):
        ramp = np.stack([255 * xx / W, 255 * yy / H, 255 * (xx + yy) / (H + W)], axis=2)
        img = np.clip(ramp + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=85, subsampling=2)
        out.append(buf.getvalue())
        mask = ((((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2) / (W / 4)) ** 2 < 1) * 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(mask).save(buf, "JPEG", quality=90)
        segs.append(buf.getvalue())
    return out, segs, "Pillow-encoded 200 x 300 ramp plus noise, quality 85, 4:2:0", Image


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    a = ap.parse_args()
    B = a.batch
    streams, segs, what, Image = make_streams(B)
    res = {"batch": B, "streams": what, "stream_bytes_mean": float(np.mean([len(s) for s in streams])), "encoder_backward_b64_ms": ENCODER_BACKWARD_B64_MS}
    for th in (1, 8, 16):
        res["entropy_ms_threads%d" % th] = wall_ms(lambda: jpeg.entropy_decode(streams, 3, threads=th))
    coef, table, totals = jpeg.entropy_decode(streams, 3, threads=8)
    n = coef.shape[0]
    pinned = torch.empty(2 * n + table.nbytes, dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:2 * n] = coef.view(np.uint8)
    pinned.numpy()[2 * n:] = table.view(np.uint8)
    staged = torch.empty(pinned.numel(), dtype=torch.uint8, device="cuda")
    workspace = torch.empty(int(totals[1]), dtype=torch.uint8, device="cuda")
    out = torch.empty(int(totals[2]), dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res["h2d_bytes"] = int(pinned.numel())
    res["h2d_ms"] = event_ms(lambda: staged.copy_(pinned, non_blocking=True), a.iters)

    def backend():
        _lib.check(lib.hpe_jpeg_backend(table.ctypes.data_as(C.c_void_p), staged.data_ptr() + 2 * n, B, staged.data_ptr(), n, workspace.data_ptr(),
                                        workspace.numel(), out.data_ptr(), out.numel(), st))

    res["backend_ms"] = event_ms(backend, a.iters)
    res["frame_bytes"] = int(totals[2])
    res["decode_jpeg_batch_wall_ms"] = wall_ms(lambda: (hpe_amd.decode_jpeg_batch(streams, 3, threads=8), torch.cuda.synchronize()))
    if segs:
        H, W = int(table["H"][0]), int(table["W"][0])
        rng = np.random.RandomState(1)
        kp = np.concatenate([rng.uniform(0, W, (B, 19, 1)), rng.uniform(0, H, (B, 19, 1)), np.ones((B, 19, 1))], axis=2).astype(np.float32)
        recs = [{"image": s, "seg": g, "height": H, "width": W, "center": np.array([W // 2, H // 2]), "filename": b"", "kp": k}
                for s, g, k in zip(streams, segs, kp)]
        draws = hpe_amd.draw_augmentation(B, generator=torch.Generator().manual_seed(0))
        res["load_training_batch_wall_ms"] = wall_ms(lambda: (hpe_amd.load_training_batch(recs, draws=draws), torch.cuda.synchronize()))
    else:
        res["load_training_batch_wall_ms"] = "NOT MEASURED"
    if Image is not None:
        def pil_one(s):
            return np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))

        for th in (1, 8):
            with ThreadPoolExecutor(max_workers=th) as ex:
                res["pillow_decode_ms_threads%d" % th] = wall_ms(lambda: list(ex.map(pil_one, streams)))
        with ThreadPoolExecutor(max_workers=8) as ex:
            def pil_all():
                frames = list(ex.map(pil_one, streams))
                host = torch.from_numpy(np.stack(frames)).pin_memory()
                host.to("cuda", non_blocking=True)
                torch.cuda.synchronize()

            res["pillow_decode_and_upload_wall_ms_threads8"] = wall_ms(pil_all)
    else:
        res["pillow_decode_ms_threads8"] = res["pillow_decode_and_upload_wall_ms_threads8"] = "NOT MEASURED"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
