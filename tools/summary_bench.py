"""What an image step of the training summaries costs (DESIGN.md "Training summaries"), beside one ``Trainer.train_step`` at the same
batch in the same run.  Rows: one ``hpe_png_filter`` launch on six 672 x 672 x 3 panels (the reference's six ``vis_images`` at three
stages); the whole ``encode_png_batch`` of those panels split into filter, the copy of the scanlines to pinned memory and deflate;
``draw_results`` with its two render calls and ``draw_panels`` alone; ``Trainer.draw_rows`` (SMPL of the shown rows, render, compose,
encode) to host-complete; and the train step.  Prints one JSON line and writes profiles/summary_bench.json.  Nothing is gated: image
steps come once per ``log_img_step`` (default 1000) steps.

    python tools/summary_bench.py [--iters 10] [--out profiles/summary_bench.json]

Timing as tools/png_bench.py: host passes are wall time, median of 5 runs after one warm-up; device work is device events around
``iters`` back-to-back calls after 3 warm-up calls, median of 5 such groups.  Synthetic full-size weights and a synthetic face list; the
panels that are encoded are the ones ``draw_results`` produced from random crops, so their rows are as hard to filter and deflate as
noise makes them -- real crops compress better."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import hpe_amd  # noqa: E402
from hpe_amd import _lib, batch_io, png_encode, synthetic  # noqa: E402
from hpe_amd.draw import draw_panels, draw_results  # noqa: E402

B, STAGES, S = 6, 3, 224


def wall_ms(fn, runs=5):
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_bench.json"))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    faces = os.path.join(tmp, "smpl_faces.npy")
    np.save(faces, synthetic.make_faces())
    w = dict(synthetic.make_encoder_params())
    w.update(synthetic.make_regressor_params(variant="bounded"))
    w.update(synthetic.make_critic_params())
    cfg = types.SimpleNamespace(batch_size=B, smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params(), weights=w,
                                smpl_face_path=faces, use_validation=False)
    tr = hpe_amd.Trainer(cfg, [], [], generator=torch.Generator(device="cuda").manual_seed(1))
    g = torch.Generator(device="cuda").manual_seed(2)
    images = torch.rand((B, S, S, 3), generator=g, device="cuda") * 2 - 1
    segs = (torch.rand((B, S, S), generator=g, device="cuda") > 0.5).float()
    kp = torch.cat([torch.rand((B, 19, 2), generator=g, device="cuda") * 1.2 - 0.6, torch.ones((B, 19, 1), device="cuda")], 2)
    th = torch.from_numpy(synthetic.make_thetas(B * STAGES, seed=9)).cuda()
    real = hpe_amd.mocap_real(tr.engine, th[:, 3:75].contiguous(), th[:, 75:].contiguous())
    res = {"batch": B, "stages": STAGES, "panels": "%d x [%d, %d, 3]" % (B, STAGES * S, 3 * S), "iters": args.iters}

    res["train_step_ms"] = event_ms(lambda: tr.train_step(images, segs, kp, *real), max(2, args.iters // 3))
    result = tr.train_step(images, segs, kp, *real)
    rows = list(range(B))

    # draw_results with and without the two render calls
    flat = torch.stack([t for t in result["thetas"]], 1).reshape(-1, 85).contiguous()
    outs = [tr.engine.smpl(flat[lo:lo + B].contiguous(), want=("verts", "kp2d")) for lo in range(0, flat.shape[0], B)]
    verts = torch.cat([o["verts"] for o in outs]).reshape(B, STAGES, -1, 3)
    kps = torch.cat([o["kp2d"] for o in outs]).reshape(B, STAGES, 19, 2)
    cams = flat[:, :3].reshape(B, STAGES, 3)
    renderer = tr.predictor.renderer
    res["draw_results_ms"] = event_ms(lambda: draw_results(renderer, images, segs, kp, verts, kps, cams), args.iters)
    rend = torch.randint(0, 256, (B * STAGES, S, S, 3), dtype=torch.uint8, device="cuda")
    res["draw_panels_ms"] = event_ms(lambda: draw_panels(images, kp, kps, rend, rend), args.iters)
    res["render_calls_ms"] = res["draw_results_ms"] - res["draw_panels_ms"]
    panels = draw_results(renderer, images, segs, kp, verts, kps, cams)

    # the encoder on those panels: filter, copy, deflate
    buf, shapes, offsets = batch_io.pack_frames(panels, png_encode.COLOR_TYPE)
    table, scan_bytes = png_encode.filter_table(shapes, offsets)
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    scan = torch.empty(scan_bytes, dtype=torch.uint8, device="cuda")
    lib, st = _lib.load(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res["png_filter_ms"] = event_ms(lambda: _lib.check(lib.hpe_png_filter(table.ctypes.data_as(C.c_void_p), table_dev.data_ptr(), B, buf.data_ptr(),
                                                                         buf.numel(), scan.data_ptr(), scan.numel(), st)), args.iters)
    res["frame_bytes"], res["scanline_bytes"] = int(buf.numel()), int(scan_bytes)
    host = torch.empty(scan_bytes, dtype=torch.uint8, pin_memory=True)
    res["scanline_copy_ms"] = wall_ms(lambda: host.copy_(scan, non_blocking=True))
    for threads in (1, 6, 16):
        res["deflate_ms_threads%d" % threads] = wall_ms(lambda: png_encode.deflate_batch(host.numpy(), table, 6, threads))
    res["encode_png_batch_wall_ms"] = wall_ms(lambda: hpe_amd.encode_png_batch(panels))
    streams = hpe_amd.encode_png_batch(panels)
    res["stream_bytes_mean"] = float(np.mean([len(s) for s in streams]))
    hist = np.zeros(5, np.int64)
    for e in table:
        o, H, rb = int(e["scan_offset"]), int(e["H"]), int(e["W"]) * int(e["C"])
        hist += np.bincount(host.numpy()[o:o + H * (rb + 1)].reshape(H, rb + 1)[:, 0], minlength=5)[:5]
    res["rows_by_filter_type"] = hist.tolist()
    back = hpe_amd.decode_png_batch(streams, channels=3)
    res["decodes_to_the_panels"] = all(torch.equal(f, p) for f, p in zip(back.frames, panels))

    # the whole image step, to host-complete PNG streams
    res["image_step_wall_ms"] = wall_ms(lambda: tr.draw_rows(images, segs, kp, rows, thetas=result["thetas"]))
    res["image_step_over_train_step"] = res["image_step_wall_ms"] / res["train_step_ms"]
    res["amortised_over_log_img_step_1000"] = res["image_step_over_train_step"] / 1000.0
    tr.engine.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
