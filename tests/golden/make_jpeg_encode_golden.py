"""Writes tests/golden/jpeg_enc/: seeded source pixels (<name>.npy), the stream Pillow's libjpeg-turbo encodes from them (<name>.jpg,
``quality=..., subsampling=..., dpi=(300, 300)``) and what Pillow decodes from that stream (<name>.dec.npy); for the dataset writer,
Pillow's re-encode of channel 0 of the committed PNG masks (seg_<mask>.jpg / .dec.npy).  tests/golden/mat5/ gets the label fixtures
of mat5_lite, written by scipy.  Needs Pillow and scipy; the tests need neither.

    python tests/golden/make_jpeg_encode_golden.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_encode_ref as R  # noqa: E402

OUT, PNG, MAT = os.path.join(HERE, "jpeg_enc"), os.path.join(HERE, "png"), os.path.join(HERE, "mat5")
CONTENT = {"noise_q30_24x40": "noise", "noise_q100_16x24": "noise", "mask_37x43": "mask", "ramp_q85_97x130": "smooth"}
MASKS = ("rec_mask_37x43", "rec_mask_31x47")


def content(kind, H, W, C, rng):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "noise":
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "mask":
        inside = ((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2) / (W / 4)) ** 2 < 1
        return (inside * 255).astype(np.uint8)
    ramp = np.stack([255 * xx / max(W - 1, 1), 255 * yy / max(H - 1, 1), 255 * (xx + yy) / max(H + W - 2, 1)], axis=2)
    img = np.clip(ramp + rng.normal(0, 4 if kind == "smooth" else 20, (H, W, 3)), 0, 255).astype(np.uint8)
    return img[:, :, 1] if C == 1 else img


def save(name, img, **args):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", dpi=(300, 300), **args)
    data = buf.getvalue()
    assert len(data) < 6144, (name, len(data))
    with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
        f.write(data)
    dec = np.asarray(Image.open(io.BytesIO(data)))
    assert dec.shape == img.shape and dec.dtype == np.uint8
    np.save(os.path.join(OUT, name + ".dec.npy"), dec)
    return data


def mat_fixtures():
    import scipy.io as sio

    os.makedirs(MAT, exist_ok=True)
    rng = np.random.RandomState(7)
    joints = rng.uniform(0, 200, (3, 14, 5))
    joints[2] = rng.randint(0, 2, (14, 5))
    sio.savemat(os.path.join(MAT, "joints.mat"), {"joints": joints})
    sio.savemat(os.path.join(MAT, "joints_compressed.mat"), {"joints": joints, "count": np.arange(6, dtype=np.int32).reshape(2, 3)}, do_compression=True)
    sio.savemat(os.path.join(MAT, "small_types.mat"), {"u8": np.arange(12, dtype=np.uint8).reshape(3, 4), "f32": np.linspace(-1, 1, 6, dtype=np.float32).reshape(2, 3),
                                                       "i16": np.array([[-3, 70000 % 30000, 5]], np.int16)})
    sio.savemat(os.path.join(MAT, "struct.mat"), {"s": {"a": np.eye(2), "b": np.ones(3)}})
    sio.savemat(os.path.join(MAT, "cell.mat"), {"c": np.array([np.eye(2), np.ones(3)], dtype=object)})
    np.savez(os.path.join(MAT, "expected.npz"), joints=joints, count=np.arange(6, dtype=np.int32).reshape(2, 3), u8=np.arange(12, dtype=np.uint8).reshape(3, 4),
             f32=np.linspace(-1, 1, 6, dtype=np.float32).reshape(2, 3), i16=np.array([[-3, 70000 % 30000, 5]], np.int16))


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.RandomState(20241)
    for name, (H, W, C, quality, sub) in R.CASES.items():
        img = content(CONTENT.get(name, "ramp"), H, W, C, rng)
        assert img.shape == ((H, W, 3) if C == 3 else (H, W))
        np.save(os.path.join(OUT, name + ".npy"), img)
        args = dict(quality=quality)
        if C == 3:
            args["subsampling"] = sub
        data = save(name, img, **args)
        mine = R.encode(img, quality, sub)
        assert mine == data, "%s: the restatement and Pillow disagree (%d vs %d bytes)" % (name, len(mine), len(data))
    for mask in MASKS:
        px = np.asarray(Image.open(os.path.join(PNG, mask + ".png")))
        px = px if px.ndim == 2 else px[:, :, 0]
        data = save("seg_" + mask, np.ascontiguousarray(px), quality=95)
        assert R.encode(px, 95) == data
    mat_fixtures()
    print("wrote %d streams" % (len(R.CASES) + len(MASKS)))


if __name__ == "__main__":
    main()
