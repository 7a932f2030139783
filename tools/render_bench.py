"""Mesh renderer timing (hpe_render): prints one JSON line.

Cases: one 640 x 480 frame (H x W) with a background -- the preview.py case, whose webcam frame is rotated by 90 degrees before
prediction --, a batch of 256 crops at 224 x 224, and the same batch rotated by 60 degrees about y (SMPLRenderer.rotated).  Meshes are
synthetic SMPL bodies from Predictor.predict -> get_original ("bounded" regressor: the camera scale stays near the mean, so the bodies
are in view).  HIP-event timing after warm-up; per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.

    python tools/render_bench.py [--iters N]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import hpe_amd
from hpe_amd import synthetic


class _Cfg(object):
    img_size = 224
    num_stage = 3
    batch_size = 8
    data_format = "NHWC"
    checkpoint_dir = None
    smpl_model_path = None


def _time(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    p = hpe_amd.Predictor(_Cfg(), smpl_model=synthetic.make_smpl_model(), mean_params=synthetic.make_mean_params(),
                          encoder_params=synthetic.make_encoder_params(), regressor_params=synthetic.make_regressor_params(variant="bounded"))
    faces = synthetic.make_faces(0)
    g = np.random.default_rng(0)
    frame = g.integers(0, 256, (640, 480, 3), dtype=np.uint8)
    crop, proc, _ = hpe_amd.preprocess_image(frame)
    imgs = torch.as_tensor(synthetic.make_images(8, seed=11)).cuda()
    imgs[0] = crop
    r = p.predict(imgs)
    cfr, vs, _ = hpe_amd.get_original(proc, r["generated_verts"][0], r["generated_cams"][0], r["generated_kp2d"][0])
    # 256 crop-space bodies: the 8 predicted ones, jittered
    B = 256
    _, v8, _ = hpe_amd.get_original({"img_size": 224, "scale": 1.0, "start_pt": [112, 112]}, r["generated_verts"], r["generated_cams"],
                                    r["generated_kp2d"])
    vb = v8[torch.as_tensor(np.arange(B) % 8).cuda()] + torch.as_tensor(g.normal(0, 0.02, (B, 1, 3)).astype(np.float32)).cuda()
    vb = vb.contiguous()
    rend = hpe_amd.SMPLRenderer(faces=faces, max_batch=B)
    frame_t = torch.as_tensor(frame).cuda()[None].contiguous()
    cam1 = torch.as_tensor(cfr)[None]
    res = {"tool": "render_bench", "faces": int(len(faces)), "verts": int(vs.shape[0]), "iters": args.iters}
    cases = {
        "frame_640x480_bg": lambda alpha=False: rend(vs[None], cam1, frame_t, alpha),
        "b256_224": lambda alpha=False: rend(vb, None, None, alpha, img_size=(224, 224)),
        "b256_224_rotated": lambda alpha=True: rend.rotated(vb, 60, None, img_size=(224, 224), do_alpha=alpha),
    }
    for name, fn in cases.items():
        ms = _time(fn, args.iters)
        # covered pixels: the alpha channel of a white-background render marks them
        if name == "frame_640x480_bg":
            covered = int((rend(vs[None], cam1, None, True)[..., 3] > 0).sum())
        elif name == "b256_224":
            covered = int((rend(vb, None, None, True, img_size=(224, 224))[..., 3] > 0).sum())
        else:
            covered = int((fn(True)[..., 3] > 0).sum())
        res[name] = {"ms": round(ms, 4), "covered_px": covered, "covered_px_per_s": round(covered / (ms * 1e-3), 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
