"""NumPy restatement of the JPEG back end (DESIGN.md "Training records and JPEG decode") from coefficients: dequantisation, libjpeg's
ISLOW inverse DCT (jidctint.c), fancy chroma upsampling (jdsample.c) and YCbCr -> RGB (jdcolor.c), all in integers.  It shares no code
with csrc/jpeg_decode.hip and takes the coefficient buffer and one table entry (hpe_amd.jpeg.TABLE_DTYPE) as the library produced them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg")
# name -> refused?  (the decodable ones carry <name>.c3.npy and <name>.c1.npy beside <name>.jpg)
CASES = ("s444_19x21", "s422_17x35", "s420_37x43", "s420_opt_33x18", "s420_rstblocks_40x50", "s422_rstrows_31x47", "grey_23x9",
         "q100_16x24", "s420_5x4", "s420_3x5", "s420_1x1", "s422_9x4", "s420_q30_97x130", "noise_q100_48x48")
REFUSED = ("progressive_24x24",)
SMALLEST_COLOUR = "s420_1x1"


def stream(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def golden(name, channels):
    return np.load(os.path.join(GOLDEN, "%s.c%d.npy" % (name, channels)))


def _wrap32(x):
    return ((x + (1 << 31)) % (1 << 32)) - (1 << 31)


def _idct8(v, shift):
    """v: the 8 inputs (int64 arrays) -> the 8 outputs, 32-bit wrap then an arithmetic shift"""
    i0, i1, i2, i3, i4, i5, i6, i7 = v
    z1 = (i2 + i6) * 4433
    tmp2, tmp3 = z1 - i6 * 15137, z1 + i2 * 6270
    tmp0, tmp1 = (i0 + i4) << 13, (i0 - i4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    outs = (tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3)
    return [_wrap32(o + (1 << (shift - 1))) >> shift for o in outs]


def plane(coef, entry, c):
    """component c's uint8 sample plane [8 * blocks_h, 8 * blocks_w]"""
    bh, bw = int(entry["blocks_h"][c]), int(entry["blocks_w"][c])
    o = int(entry["coef_offset"][c])
    blk = coef[o:o + 64 * bh * bw].astype(np.int64).reshape(bh * bw, 8, 8) * entry["quant"][c].astype(np.int64).reshape(1, 8, 8)
    ws = np.stack(_idct8([blk[:, r, :] for r in range(8)], 11), axis=1)  # pass 1 down the columns: [block, row, column]
    px = np.stack(_idct8([ws[:, :, x] for x in range(8)], 18), axis=2)  # pass 2 along the rows
    px = np.clip(px + 128, 0, 255).astype(np.uint8)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2(rows, n, near_w, far_w, r_even, r_odd, shift):
    """the horizontal triangle filter of jdsample.c on int rows [*, n] -> [*, 2n]"""
    out = np.zeros((rows.shape[0], 2 * n), np.int64)
    total = near_w + far_w
    out[:, 0] = (total * rows[:, 0] + r_even) >> shift
    out[:, 2 * n - 1] = (total * rows[:, n - 1] + r_odd) >> shift
    out[:, 2:2 * n:2] = (near_w * rows[:, 1:] + far_w * rows[:, :-1] + r_even) >> shift
    out[:, 1:2 * n - 1:2] = (near_w * rows[:, :-1] + far_w * rows[:, 1:] + r_odd) >> shift
    return out


def upsample(p, H, W, hmax, vmax):
    """a chroma plane to [H, W]"""
    if hmax == 1:
        return p[:H, :W].astype(np.int64)
    n, m = -(-W // hmax), -(-H // vmax)
    src = p[:m, :n].astype(np.int64)
    if n <= 2:  # libjpeg takes the fancy filters only above 2 columns: plain replication
        return np.repeat(np.repeat(src, vmax, axis=0), 2, axis=1)[:H, :W]
    if vmax == 1:
        out = _h2(src, n, 3, 1, 1, 2, 2)
        out[:, 0], out[:, 2 * n - 1] = src[:, 0], src[:, n - 1]
        return out[:H, :W]
    y = np.arange(2 * m)
    r = y >> 1
    far = np.where(y & 1, np.minimum(r + 1, m - 1), np.maximum(r - 1, 0))
    s = 3 * src[r] + src[far]
    return _h2(s, n, 3, 1, 8, 7, 4)[:H, :W]


def decode(coef, entry):
    """one table entry -> uint8 [H,W,3] or [H,W,1]"""
    H, W, ch, ncomp = int(entry["H"]), int(entry["W"]), int(entry["channels"]), int(entry["ncomp"])
    y = plane(coef, entry, 0)[:H, :W].astype(np.int64)
    if ncomp == 1:
        return np.repeat(y[:, :, None], ch, axis=2).astype(np.uint8)
    hmax, vmax = int(entry["hmax"]), int(entry["vmax"])
    cb = upsample(plane(coef, entry, 1), H, W, hmax, vmax) - 128
    cr = upsample(plane(coef, entry, 2), H, W, hmax, vmax) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)
