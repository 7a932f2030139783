"""Checkpoint-score timing (hpe_eval_scores): prints one JSON line, and writes it to --out when given.

256 crops of 224 x 224 with the synthetic body (6890 vertices, the 13776 faces of synthetic.make_faces): the vertices and keypoints of all
three IEF stages come from one real forward of 8 images, repeated with a jitter of a few pixels.  Timed with HIP events after 5 warm-up
calls, median of 5 groups of 50 calls: hpe_eval_scores (both parts) with n_stage = 1 and 3, called as the library is (preallocated
outputs) and through metrics.eval_scores, and in the same process hpe_render with do_alpha on the same bodies, the only way to a
silhouette without this call.  Counters, if wanted, come from a separate run under the profiler.

    python tools/eval_scores_bench.py [--out profiles/eval_scores_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import hpe_amd
from hpe_amd import _lib, metrics, synthetic

B, S, WARMUP, GROUPS, CALLS = 256, 224, 5, 5, 50


class _Cfg(object):
    img_size = S
    num_stage = 3
    batch_size = 8
    data_format = "NHWC"
    checkpoint_dir = None
    smpl_model_path = None


def timed(fn):
    """-> (median, min, max) ms per call over GROUPS groups of CALLS calls"""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    groups = []
    for _ in range(GROUPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        groups.append(e0.elapsed_time(e1) / CALLS)
    return [round(float(x), 5) for x in (np.median(groups), min(groups), max(groups))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    p = hpe_amd.Predictor(_Cfg(), smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params(),
                          encoder_params=synthetic.make_encoder_params(), regressor_params=synthetic.make_regressor_params(variant="bounded"))
    faces_np = synthetic.make_faces(0)
    g = np.random.default_rng(0)
    imgs = torch.as_tensor(synthetic.make_images(8, seed=11)).cuda()
    stages = p.engine.forward(imgs, all_stages=True, want=("verts", "cams", "kp2d", "verts2d"))
    rows = torch.as_tensor(np.arange(B) % 8).cuda()
    shift = torch.as_tensor(g.normal(0, 3.0, (B, 1, 2)).astype(np.float32)).cuda()
    verts2d = [(st["verts2d"][rows] + shift).contiguous() for st in stages]
    kp2d = [st["kp2d"][rows].contiguous() for st in stages]
    kp_gt = torch.cat([kp2d[-1] + 0.05, torch.ones(B, 19, 1, device="cuda")], 2).contiguous()
    yy, xx = np.mgrid[:S, :S]
    seg = torch.as_tensor((((xx - 112) / 50.0) ** 2 + ((yy - 112) / 90.0) ** 2 <= 1.0).astype(np.float32)).cuda()[None].repeat(B, 1, 1).contiguous()
    faces = metrics.upload_faces(faces_np, 6890, "cuda")
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"tool": "eval_scores_bench", "B": B, "H": S, "W": S, "verts": 6890, "faces": int(len(faces_np)), "warmup": WARMUP, "groups": GROUPS,
           "calls_per_group": CALLS, "ms": "median, min, max over the groups"}
    for n in (1, 3):
        counts = torch.empty((n, B, 4), dtype=torch.int32, device="cuda")
        err = torch.empty((n, B, 19), device="cuda")
        norm = torch.empty((B, 2), device="cuda")
        vp = (C.c_void_p * n)(*[t.data_ptr() for t in verts2d[3 - n:]])
        kp = (C.c_void_p * n)(*[t.data_ptr() for t in kp2d[3 - n:]])

        def call():
            _lib.check(lib.hpe_eval_scores(vp, faces.data_ptr(), len(faces_np), seg.data_ptr(), kp_gt.data_ptr(), kp, n, B, 6890, 19, S, S,
                                           counts.data_ptr(), err.data_ptr(), norm.data_ptr(), st))

        res["eval_scores_n%d_ms" % n] = timed(call)
        res["eval_scores_n%d_wrapper_ms" % n] = timed(lambda: metrics.eval_scores(verts2d[3 - n:], faces, seg, kp_gt, kp2d[3 - n:]))
        res["eval_scores_n%d_silhouette_only_ms" % n] = timed(lambda: _lib.check(lib.hpe_eval_scores(
            vp, faces.data_ptr(), len(faces_np), seg.data_ptr(), None, None, n, B, 6890, 19, S, S, counts.data_ptr(), None, None, st)))
        c = counts[-1].double().sum(0).cpu().numpy()
        res["n%d_last_stage" % n] = {"covered_px_per_image": round(float(c[0] + c[1]) / B, 1), "iou": round(float(c[0] / (c[0] + c[1] + c[2])), 4)}
    # how the faces split between the two walks (last stage, the kernel's own box rule)
    v = verts2d[-1][:8].cpu().numpy().astype(np.float64)
    tri = np.rint(256.0 * v[:, faces_np])  # [8,F,3,2]
    lo, hi = tri.min(2), tri.max(2)
    x0, x1 = np.maximum(np.ceil(lo[..., 0] / 256), 0), np.minimum(np.floor(hi[..., 0] / 256), S - 1)
    y0, y1 = np.maximum(np.ceil(lo[..., 1] / 256), 0), np.minimum(np.floor(hi[..., 1] / 256), S - 1)
    box = np.where((x0 <= x1) & (y0 <= y1), (x1 - x0 + 1) * (y1 - y0 + 1), 0)
    res["boxes_per_image"] = {"empty": round(float((box == 0).sum(1).mean()), 1), "own_lane": round(float(((box > 0) & (box <= 64)).sum(1).mean()), 1),
                              "wave": round(float((box > 64).sum(1).mean()), 1), "samples": round(float(box.sum(1).mean()), 1),
                              "largest": int(box.max())}
    # the renderer on the same bodies: crop-space meshes as render_bench builds them
    _, v8, _ = hpe_amd.get_original({"img_size": S, "scale": 1.0, "start_pt": [112, 112]}, stages[-1]["verts"], stages[-1]["cams"], stages[-1]["kp2d"])
    vb = v8[rows].contiguous()
    rend = hpe_amd.SMPLRenderer(faces=faces_np, max_batch=B)
    res["render_do_alpha_ms"] = timed(lambda: rend(vb, None, None, True, img_size=(S, S)))
    res["render_covered_px_per_image"] = round(float((rend(vb, None, None, True, img_size=(S, S))[..., 3] > 0).sum()) / B, 1)
    res["render_over_eval_scores_n1"] = round(res["render_do_alpha_ms"][0] / res["eval_scores_n1_ms"][0], 2)
    res["render_x3_over_eval_scores_n3"] = round(3 * res["render_do_alpha_ms"][0] / res["eval_scores_n3_ms"][0], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
