"""Writes tests/golden/jpeg/ and tests/golden/records/: synthetic JPEG streams (ramps plus noise) with the pixels Pillow's libjpeg-turbo
decodes from them for 3 channels and for 1 (Image.draft("L")), and the record files built from them.  Needs Pillow; the tests do not.

    python tests/golden/make_jpeg_golden.py
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import records_writer as RW  # noqa: E402

JPEG, RECORDS = os.path.join(HERE, "jpeg"), os.path.join(HERE, "records")
S444, S422, S420 = 0, 1, 2
# name (sizes are H x W) -> (H, W, save arguments, content)
CASES = {
    "s444_19x21": (19, 21, dict(quality=85, subsampling=S444), "ramp"),
    "s422_17x35": (17, 35, dict(quality=85, subsampling=S422), "ramp"),
    "s420_37x43": (37, 43, dict(quality=85, subsampling=S420), "ramp"),
    "s420_opt_33x18": (33, 18, dict(quality=80, subsampling=S420, optimize=True), "ramp"),
    "s420_rstblocks_40x50": (40, 50, dict(quality=85, subsampling=S420, restart_marker_blocks=2), "ramp"),
    "s422_rstrows_31x47": (31, 47, dict(quality=85, subsampling=S422, restart_marker_rows=1), "ramp"),
    "grey_23x9": (23, 9, dict(quality=85), "grey"),
    "q100_16x24": (16, 24, dict(quality=100, subsampling=S420), "ramp"),
    "s420_5x4": (5, 4, dict(quality=85, subsampling=S420), "ramp"),
    "s420_3x5": (3, 5, dict(quality=85, subsampling=S420), "ramp"),
    "s420_1x1": (1, 1, dict(quality=85, subsampling=S420), "ramp"),
    "s422_9x4": (9, 4, dict(quality=85, subsampling=S422), "ramp"),
    "s420_q30_97x130": (97, 130, dict(quality=30, subsampling=S420), "ramp"),
    "noise_q100_48x48": (48, 48, dict(quality=100, subsampling=S420), "noise"),
    "progressive_24x24": (24, 24, dict(quality=85, subsampling=S420, progressive=True), "ramp"),
    # masks of the image records below
    "seg_37x43": (37, 43, dict(quality=90), "mask"),
    "seg_40x50": (40, 50, dict(quality=90), "mask"),
    "seg_31x47": (31, 47, dict(quality=90), "mask"),
}


def content(kind, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "noise":
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "mask":
        inside = ((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2) / (W / 4)) ** 2 < 1
        return (inside * 255).astype(np.uint8)
    ramp = np.stack([255 * xx / max(W - 1, 1), 255 * yy / max(H - 1, 1), 255 * (xx + yy) / max(H + W - 2, 1)], axis=2)
    img = np.clip(ramp + rng.normal(0, 20, (H, W, 3)), 0, 255).astype(np.uint8)
    return img[:, :, 1] if kind == "grey" else img


def main():
    os.makedirs(JPEG, exist_ok=True)
    os.makedirs(RECORDS, exist_ok=True)
    rng = np.random.RandomState(20240)
    streams = {}
    for name, (H, W, args, kind) in CASES.items():
        buf = io.BytesIO()
        Image.fromarray(content(kind, H, W, rng)).save(buf, "JPEG", **args)
        data = buf.getvalue()
        assert len(data) < 6144, (name, len(data))
        streams[name] = data
        with open(os.path.join(JPEG, name + ".jpg"), "wb") as f:
            f.write(data)
        if name.startswith("progressive"):
            continue
        c3 = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        im = Image.open(io.BytesIO(data))
        im.draft("L", im.size)
        c1 = np.asarray(im)
        assert c3.shape == (H, W, 3) and c1.shape == (H, W) and c1.dtype == np.uint8, (name, c3.shape, c1.shape, im.mode)
        np.save(os.path.join(JPEG, name + ".c3.npy"), c3)
        np.save(os.path.join(JPEG, name + ".c1.npy"), c1)
    expected, payloads = [], []
    for i, (img, seg) in enumerate((("s420_37x43", "seg_37x43"), ("s420_rstblocks_40x50", "seg_40x50"), ("s422_rstrows_31x47", "seg_31x47"))):
        H, W = CASES[img][:2]
        x = [round(float(v), 2) for v in rng.uniform(0, W, 14)]
        y = [round(float(v), 2) for v in rng.uniform(0, H, 14)]
        vis = [int(v) for v in rng.randint(0, 2, 14)]
        face = None if i == 1 else [round(float(v), 2) for v in np.concatenate([rng.uniform(0, W, 5), rng.uniform(0, H, 5), rng.randint(0, 2, 5)])]
        center = [W // 2 + i - 1, H // 2 - i]
        fname = ("synthetic/%s.jpg" % img).encode()
        payloads.append(RW.image_example(streams[img], streams[seg], H, W, center, fname, x, y, vis, face))
        expected.append({"image": img, "seg": seg, "height": H, "width": W, "center": center, "filename": fname.decode(), "x": x, "y": y,
                         "visibility": vis, "face_pts": face})
    RW.write_tfrecords(os.path.join(RECORDS, "images.tfrecords"), payloads)
    pose = rng.normal(0, 0.3, (4, 72)).astype(np.float32)
    shape = rng.normal(0, 1.0, (4, 10)).astype(np.float32)
    RW.write_tfrecords(os.path.join(RECORDS, "mocap.tfrecords"), [RW.mocap_example(p.tolist(), s.tolist()) for p, s in zip(pose, shape)])
    np.save(os.path.join(RECORDS, "mocap_pose.npy"), pose)
    np.save(os.path.join(RECORDS, "mocap_shape.npy"), shape)
    with open(os.path.join(RECORDS, "images_expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
    print("wrote %d streams, %d image records, %d mocap rows" % (len(streams), len(payloads), len(pose)))


if __name__ == "__main__":
    main()
