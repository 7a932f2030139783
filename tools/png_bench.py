"""Where the time of decoding a batch of PNG streams goes, for the two kinds the reference's records hold: B = 64 grey 8-bit 200 x 300
masks (LSP's ``image/seg_gt``) and B = 8 RGB 1280 x 720 frames (MPII's ``image/encoded``; 8 is the reference's batch size).  Rows: the
host chunk walk + inflate (1, 8, 16 threads), the one host-to-device copy, the unfilter launch, the store launch, and the whole
``decode_png_batch`` to device-complete; beside them Pillow's decode of the same streams on the same thread counts plus the pinned
upload of the pixels -- the yardstick, since there was no PNG decoder here before.  Prints one JSON line and writes
profiles/png_bench.json.

    python tools/png_bench.py [--iters 10] [--out profiles/png_bench.json]

Timing as tools/jpeg_bench.py: host passes are wall time, median of 5 runs after one warm-up; device work is device events around
`iters` back-to-back calls after 3 warm-up calls, median of 5 such groups.  Masks asked for 1 channel and frames asked for 3 are direct
images (launch one writes the frame, launch two is not launched), so ``unfilter_ms`` is hpe_png_backend on that request; ``unfilter_ms_every_row_paeth`` is the same launch on the last image of the batch re-encoded with Paeth on every row; the store is
measured on the other request (masks to 3 channels, frames to 1), as that call's time less the unfilter's.  The streams are encoded
with Pillow when it is importable, so the filters are the ones its encoder picks; without it tests/png_writer.py writes them with the Up
filter on every row and the JSON says so."""
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
from hpe_amd import _lib, png  # noqa: E402


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


def make_streams(kind, B):
    try:
        from PIL import Image
    except ImportError:
        Image = None
    rng = np.random.RandomState(11)
    out = []
    for i in range(B):
        if kind == "masks":
            H, W = 200, 300
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
            img = ((((yy - H / 2 - i % 7) / (H / 3)) ** 2 + ((xx - W / 2 + i % 5) / (W / 4)) ** 2 < 1) * 255).astype(np.uint8)
        else:
            H, W = 720, 1280
            yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
            ramp = np.stack([255 * xx / W, 255 * yy / H, 255 * (xx + yy) / (H + W)], axis=2)
            img = np.clip(ramp + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
        if Image is not None:
            buf = io.BytesIO()
            Image.fromarray(img).save(buf, "PNG")
            out.append(buf.getvalue())
        else:
            import png_writer as PW

            out.append(PW.write_png(img.reshape(H, W, -1), 0 if kind == "masks" else 2, 8, 2))
    return out, ("Pillow-encoded" if Image is not None else "png_writer, Up filter on every row"), Image, img


def filter_histogram(streams):
    hist = np.zeros(5, np.int64)
    staged, table, _ = png.inflate_batch(streams, 3, threads=8)
    for e in table:
        H, rb, o = int(e["H"]), int(e["rowbytes"]), int(e["raw_offset"])
        hist += np.bincount(staged[o:o + H * (rb + 1)].reshape(H, rb + 1)[:, 0], minlength=5)[:5]
    return hist.tolist()


def measure(kind, B, native, iters):
    streams, how, Image, last = make_streams(kind, B)
    other = 4 - native
    res = {"batch": B, "streams": how, "stream_bytes_mean": float(np.mean([len(s) for s in streams])), "channels": native,
           "rows_by_filter_type": filter_histogram(streams)}
    for th in (1, 8, 16):
        res["host_parse_inflate_ms_threads%d" % th] = wall_ms(lambda: png.inflate_batch(streams, native, threads=th))
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def backend_of(channels):
        staged, table, totals = png.inflate_batch(streams, channels, threads=8)
        pinned = torch.empty(staged.size, dtype=torch.uint8, pin_memory=True)
        pinned.numpy()[:] = staged
        dev = torch.empty(staged.size, dtype=torch.uint8, device="cuda")
        dev.copy_(pinned)
        workspace = torch.empty(int(totals[1]), dtype=torch.uint8, device="cuda")
        out = torch.empty(int(totals[2]), dtype=torch.uint8, device="cuda")
        raw = int(totals[0])

        def run():
            _lib.check(lib.hpe_png_backend(table.ctypes.data_as(C.c_void_p), dev.data_ptr() + raw, B, dev.data_ptr(), raw, workspace.data_ptr(),
                                           workspace.numel(), out.data_ptr(), out.numel(), st))

        return run, pinned, dev, int(totals[2]), int(totals[3]), (table, workspace, out)

    run, pinned, dev, frame_bytes, groups, keep = backend_of(native)
    assert groups == 0  # direct images: the unfilter launch alone
    res["h2d_bytes"] = int(pinned.numel())
    res["h2d_ms"] = event_ms(lambda: dev.copy_(pinned, non_blocking=True), iters)
    res["unfilter_ms"] = event_ms(run, iters)
    res["frame_bytes"] = frame_bytes
    # the same launch when every row is Paeth (the encoder above picks what it likes; a strip with a Paeth row runs the longer body)
    import png_writer as PW

    one = PW.write_png(last.reshape(last.shape[0], last.shape[1], -1), 0 if kind == "masks" else 2, 8, 4, level=1)
    streams, keep_streams = [one] * B, streams
    run4, _, _, _, _, keep4 = backend_of(native)
    res["unfilter_ms_every_row_paeth"] = event_ms(run4, iters)
    streams = keep_streams
    run2, _, _, _, groups2, keep2 = backend_of(other)
    assert groups2 > 0
    res["backend_ms_channels%d" % other] = event_ms(run2, iters)
    res["store_ms_channels%d" % other] = res["backend_ms_channels%d" % other] - res["unfilter_ms"]
    res["decode_png_batch_wall_ms"] = wall_ms(lambda: (hpe_amd.decode_png_batch(streams, native, threads=8), torch.cuda.synchronize()))
    res["device_share_of_call"] = (res["h2d_ms"] + res["unfilter_ms"]) / res["decode_png_batch_wall_ms"]
    res["unfilter_over_inflate_threads8"] = res["unfilter_ms"] / res["host_parse_inflate_ms_threads8"]
    if Image is not None:
        mode = "L" if native == 1 else "RGB"

        def pil_one(s):
            return np.asarray(Image.open(io.BytesIO(s)).convert(mode))

        got = hpe_amd.decode_png_batch(streams, native, threads=8).frames
        res["equals_pillow"] = all(np.array_equal(g.cpu().numpy(), pil_one(s)) for g, s in zip(got, streams))
        for th in (1, 8, 16):
            with ThreadPoolExecutor(max_workers=th) as ex:
                res["pillow_decode_ms_threads%d" % th] = wall_ms(lambda: list(ex.map(pil_one, streams)))

                def pil_all():
                    frames = list(ex.map(pil_one, streams))
                    host = torch.from_numpy(np.stack(frames)).pin_memory()
                    host.to("cuda", non_blocking=True)
                    torch.cuda.synchronize()

                res["pillow_decode_and_upload_wall_ms_threads%d" % th] = wall_ms(pil_all)
        res["decode_png_batch_over_pillow_and_upload_threads8"] = res["decode_png_batch_wall_ms"] / res["pillow_decode_and_upload_wall_ms_threads8"]
    else:
        res["pillow_decode_ms_threads8"] = res["pillow_decode_and_upload_wall_ms_threads8"] = "NOT MEASURED"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_bench.json"))
    a = ap.parse_args()
    res = {"masks_200x300_grey8_b64": measure("masks", 64, 1, a.iters), "frames_1280x720_rgb8_b8": measure("frames", 8, 3, a.iters)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
