"""Writes tests/golden/png/ and tests/golden/records/images_png.tfrecords: synthetic PNG streams through tests/png_writer.py, seeded, so
that ``case(name)`` gives again the very array a committed stream was written from -- the array is the truth, PNG is lossless -- and
a record file whose three records mix PNG and JPEG streams (the JPEG ones are the committed fixtures of tests/golden/jpeg/).

    python tests/golden/make_png_golden.py
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import png_writer as PW  # noqa: E402

PNG, JPEG, RECORDS = os.path.join(HERE, "png"), os.path.join(HERE, "jpeg"), os.path.join(HERE, "records")
CYCLE = "cycle"  # filters 4, 3, 2, 1, 0 per row: Paeth on row 0, where Prior is all zeros
# name -> (H, W, colour type, depth, filters, content, further write_png arguments)
CASES = {
    # 8-bit: bpp 1, 2, 3, 4; heights 1, 2, 63, 64, 65, 130 (a strip boundary, a third strip); widths 1, 2, 3, 5, 67
    "g8_1x1_f0": (1, 1, 0, 8, 0, "noise", {}),
    "g8_2x3_f4": (2, 3, 0, 8, 4, "noise", {}),
    "g8_64x1_f4": (64, 1, 0, 8, 4, "noise", {}),
    "ga_63x5_f1": (63, 5, 4, 8, 1, "noise", {}),
    "rgb_64x5_f2": (64, 5, 2, 8, 2, "noise", {}),
    "rgba_65x3_f3": (65, 3, 6, 8, 3, "noise", {}),
    "rgb_130x5_f4": (130, 5, 2, 8, 4, "noise", {}),
    "rgba_130x2_cycle": (130, 2, 6, 8, CYCLE, "noise", {}),
    "g8_65x67_cycle": (65, 67, 0, 8, CYCLE, "noise", {}),
    "rgb_1x67_f1": (1, 67, 2, 8, 1, "noise", {}),
    "rgba_2x67_f3": (2, 67, 6, 8, 3, "noise", {}),
    "rgb_63x67_cycle": (63, 67, 2, 8, CYCLE, "crafted", {}),
    # flats and ramps: Paeth's pa == pc and pb == pc ties with unequal candidates, Average sums of 256 and more
    "g8_130x67_f4": (130, 67, 0, 8, 4, "crafted", {}),
    "ga_130x67_f3": (130, 67, 4, 8, 3, "crafted", {}),
    # depths 1, 2, 4 at W = 9 and W = 5: a partial last byte, bpp = 1 on packed bytes
    "g1_65x9_cycle": (65, 9, 0, 1, CYCLE, "noise", {}),
    "g2_64x5_f1": (64, 5, 0, 2, 1, "noise", {}),
    "g4_63x9_f3": (63, 9, 0, 4, 3, "noise", {}),
    "g4_2x5_f2": (2, 5, 0, 4, 2, "noise", {}),
    "p1_5x9_f0": (5, 9, 3, 1, 0, "noise", {"entries": 2}),
    "p2_65x5_f4": (65, 5, 3, 2, 4, "noise", {"entries": 4}),
    "p4_63x9_f3": (63, 9, 3, 4, 3, "noise", {"entries": 16}),
    "p8_130x5_cycle": (130, 5, 3, 8, CYCLE, "noise", {"entries": 200}),  # indices up to 255: beyond PLTE reads black
    # chunks
    "g8_5x5_idat1": (5, 5, 0, 8, CYCLE, "noise", {"idat_size": 1}),
    "rgb_3x5_idat7": (3, 5, 2, 8, 4, "noise", {"idat_size": 7}),
    "p8_2x5_trns": (2, 5, 3, 8, 1, "noise", {"entries": 7, "trns": True}),
    "rgb_2x2_ancillary": (2, 2, 2, 8, 3, "noise", {"ancillary": True}),
    # the streams of the record file
    "rec_mask_37x43": (37, 43, 0, 8, CYCLE, "mask", {}),
    "rec_mask_31x47": (31, 47, 0, 8, 4, "mask", {}),
    "rec_frame_31x47": (31, 47, 2, 8, CYCLE, "ramp", {}),
}
NAMES = tuple(n for n in CASES if not n.startswith("rec_"))
SMALLEST_COLOUR = "rgb_2x2_ancillary"


def crafted(H, W):
    """16 x 16 tiles: a flat of 200, the two ramps whose Paeth distances tie with unequal candidates (6x - 3y: pb == pc, b wins over c;
    -3x + 6y: pa == pc, a wins over c), a diagonal ramp (pa == pb), a 0 / 255 checker, a ramp that wraps mod 256"""
    yy, xx = np.mgrid[0:H, 0:W]
    ty, tx, y, x = yy // 16, xx // 16, yy % 16, xx % 16
    tiles = [np.full((H, W), 200), 100 + 6 * x - 3 * y, 100 - 3 * x + 6 * y, 2 * (x + y), 255 * ((x + y) & 1), 37 * x + 11 * y]
    kind = (tx + 2 * ty) % len(tiles)
    out = np.zeros((H, W), np.int64)
    for k, t in enumerate(tiles):
        out = np.where(kind == k, t, out)
    return (out % 256).astype(np.uint8)


def case(name):
    """-> {'samples' uint8 [H, W, spp], 'color_type', 'depth', 'palette' (uint8 [n, 3] or None), 'filters' [H], 'kwargs' of write_png}"""
    H, W, ct, depth, filters, content, extra = CASES[name]
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    spp = PW.SAMPLES[ct]
    if content == "noise":
        samples = rng.randint(0, 1 << depth, (H, W, spp)).astype(np.uint8)  # full range: the filters wrap mod 256
    elif content == "crafted":
        base = crafted(H, W)
        samples = np.stack([(base.astype(np.int64) * (k + 1) + 50 * k) % 256 for k in range(spp)], axis=2).astype(np.uint8)
    elif content == "mask":
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        samples = ((((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2) / (W / 4)) ** 2 < 1) * 255).astype(np.uint8)[:, :, None]
    else:  # ramp: a smooth frame with mild noise
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        ramp = np.stack([255 * xx / (W - 1), 255 * yy / (H - 1), 255 * (xx + yy) / (H + W - 2)], axis=2)
        samples = np.clip(ramp + rng.normal(0, 4, (H, W, 3)), 0, 255).astype(np.uint8)
    palette = rng.randint(0, 256, (extra["entries"], 3)).astype(np.uint8) if ct == 3 else None
    kwargs = {}
    if "idat_size" in extra:
        kwargs["idat_size"] = extra["idat_size"]
    if extra.get("trns"):
        kwargs["before_idat"] = [(b"tRNS", bytes(rng.randint(0, 256, 5).astype(np.uint8)))]
    if extra.get("ancillary"):
        kwargs["before_idat"] = [(b"gAMA", (45455).to_bytes(4, "big")), (b"acTL", b"\0\0\0\1\0\0\0\0")]
        kwargs["after_idat"] = [(b"tEXt", b"Comment\0a chunk between the last IDAT and IEND")]
    rows = [(4, 3, 2, 1, 0)[y % 5] for y in range(H)] if filters == CYCLE else [filters] * H
    return {"samples": samples, "color_type": ct, "depth": depth, "palette": palette, "filters": rows, "kwargs": kwargs}


def write(name):
    c = case(name)
    return PW.write_png(c["samples"], c["color_type"], c["depth"], c["filters"], c["palette"], **c["kwargs"])


def truth(name, channels):
    """what the stream decodes to: uint8 [H, W, 3] or [H, W].  Grey scales by 255 / 85 / 17 and replicates; a palette index beyond PLTE
    reads black; alpha is dropped; colour to grey is (9797 R + 19234 G + 3737 B) >> 15."""
    c = case(name)
    s, ct = c["samples"].astype(np.int64), c["color_type"]
    if ct in (0, 4):
        g = s[:, :, 0] * (255 // ((1 << c["depth"]) - 1))
        return (g if channels == 1 else np.stack([g, g, g], axis=2)).astype(np.uint8)
    if ct == 3:
        pal = np.concatenate([c["palette"].astype(np.int64), np.zeros((256 - len(c["palette"]), 3), np.int64)])
        s = pal[s[:, :, 0]]
    if channels == 3:
        return s[:, :, :3].astype(np.uint8)
    return ((9797 * s[:, :, 0] + 19234 * s[:, :, 1] + 3737 * s[:, :, 2]) // 32768).astype(np.uint8)


def main():
    import records_writer as RW

    os.makedirs(PNG, exist_ok=True)
    streams = {}
    for name in CASES:
        streams[name] = write(name)
        assert len(streams[name]) < 6144, (name, len(streams[name]))
        with open(os.path.join(PNG, name + ".png"), "wb") as f:
            f.write(streams[name])

    def jpeg(n):
        with open(os.path.join(JPEG, n + ".jpg"), "rb") as f:
            return f.read()

    rng = np.random.RandomState(20241)
    # (frame, mask): a PNG mask with a JPEG frame, a JPEG mask with a JPEG frame, a PNG mask with a PNG frame
    pairs = (("s420_37x43", "rec_mask_37x43"), ("s420_rstblocks_40x50", "seg_40x50"), ("rec_frame_31x47", "rec_mask_31x47"))
    expected, payloads = [], []
    for i, (img, seg) in enumerate(pairs):
        H, W = (CASES[img][:2] if img in CASES else tuple(int(v) for v in img.split("_")[-1].split("x")))
        x = [round(float(v), 2) for v in rng.uniform(0, W, 14)]
        y = [round(float(v), 2) for v in rng.uniform(0, H, 14)]
        vis = [int(v) for v in rng.randint(0, 2, 14)]
        face = None if i == 1 else [round(float(v), 2) for v in np.concatenate([rng.uniform(0, W, 5), rng.uniform(0, H, 5), rng.randint(0, 2, 5)])]
        center = [W // 2 + i - 1, H // 2 - i]
        fname = ("synthetic/%s" % img).encode()
        get = lambda n: streams[n] if n in streams else jpeg(n)  # noqa: E731
        payloads.append(RW.image_example(get(img), get(seg), H, W, center, fname, x, y, vis, face))
        expected.append({"image": img, "seg": seg, "height": H, "width": W, "center": center, "filename": fname.decode(), "x": x, "y": y,
                         "visibility": vis, "face_pts": face})
    RW.write_tfrecords(os.path.join(RECORDS, "images_png.tfrecords"), payloads)
    with open(os.path.join(RECORDS, "images_png_expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
    print("wrote %d streams (%d bytes), %d image records" % (len(streams), sum(len(s) for s in streams.values()), len(payloads)))


if __name__ == "__main__":
    main()
