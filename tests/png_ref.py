"""NumPy restatement of the PNG back end (DESIGN.md "PNG streams in the records") from the inflated scanlines: unfilter, unpack, palette
and channel conversion.  It shares no code with csrc/png_decode.hip and takes the staged buffer and one table entry
(hpe_amd.png.TABLE_DTYPE) as hpe_amd.png.inflate_batch produced them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png")


def stream(name):
    with open(os.path.join(GOLDEN, name + ".png"), "rb") as f:
        return f.read()


def unfilter(scan, bpp):
    """scanlines uint8 [H, 1 + rowbytes] -> rows uint8 [H, rowbytes].  Bytes left of the row and the row above row 0 read zero."""
    H, rb = scan.shape[0], scan.shape[1] - 1
    rec = np.zeros((H + 1, rb + bpp), np.int64)
    for y in range(H):
        ft, f = int(scan[y, 0]), scan[y, 1:].astype(np.int64)
        prior, cur = rec[y], rec[y + 1]
        if ft == 0:
            cur[bpp:] = f
        elif ft == 2:
            cur[bpp:] = (f + prior[bpp:]) & 255
        else:
            for i in range(rb):
                a, b, c = int(cur[i]), int(prior[i + bpp]), int(prior[i])
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                elif ft == 4:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                else:
                    raise ValueError("filter type %d" % ft)
                cur[i + bpp] = (int(f[i]) + pred) & 255
    return rec[1:, bpp:].astype(np.uint8)


def unpack(rows, W, depth, samples):
    """rows uint8 [H, rowbytes] -> sample values uint8 [H, W, samples]"""
    H = rows.shape[0]
    if depth == 8:
        return rows[:, :W * samples].reshape(H, W, samples)
    x = np.arange(W) * depth
    return ((rows[:, x >> 3] >> (8 - depth - (x & 7))) & ((1 << depth) - 1)).astype(np.uint8).reshape(H, W, 1)


def rgb_to_gray(rgb):
    """libpng's png_set_rgb_to_gray without gamma, coefficients 9797 / 19234 / 3737 of 32768, truncating"""
    v = rgb.astype(np.int64)
    return ((9797 * v[..., 0] + 19234 * v[..., 1] + 3737 * v[..., 2]) >> 15).astype(np.uint8)


def convert(samples, color_type, depth, palette, channels):
    """sample values [H, W, spp] -> uint8 [H, W, 3] or [H, W].  palette: uint8 [n, 3]; an index beyond it reads black."""
    if color_type in (0, 4):
        g = samples[:, :, 0].astype(np.int64) * {1: 255, 2: 85, 4: 17, 8: 1}[depth]
        g = g.astype(np.uint8)
        return g if channels == 1 else np.repeat(g[:, :, None], 3, axis=2)
    if color_type == 3:
        full = np.zeros((256, 3), np.uint8)
        full[:len(palette)] = palette
        rgb = full[samples[:, :, 0]]
    else:
        rgb = samples[:, :, :3]
    return rgb_to_gray(rgb) if channels == 1 else np.ascontiguousarray(rgb)


def decode(staged, entry):
    """one table entry of inflate_batch's staged buffer -> uint8 [H, W, 3] or [H, W]"""
    H, W, ct, depth, rb, bpp, ch = (int(entry[k]) for k in ("H", "W", "color_type", "depth", "rowbytes", "bpp", "channels"))
    o = int(entry["raw_offset"])
    rows = unfilter(staged[o:o + H * (rb + 1)].reshape(H, rb + 1), bpp)
    palette = None
    if ct == 3:
        p = int(entry["pal_offset"])
        palette = staged[p:p + 1024].reshape(256, 4)[:, :3]
    return convert(unpack(rows, W, depth, {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct]), ct, depth, palette, ch)
