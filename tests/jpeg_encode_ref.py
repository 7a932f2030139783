"""NumPy restatement of the JPEG encoder (DESIGN.md "Dataset writers and JPEG encode"): libjpeg's default baseline compressor -- jccolor.c,
jcsample.c without smoothing, the edge rules of jcprepct.c / jccoefct.c, jfdctint.c (JDCT_ISLOW), the standard Huffman tables -- written
from the definition and sharing no code with the package.  ``forward`` gives the coefficient planes in the decoder's layout, dummy blocks
included; ``encode`` the whole stream.  Every intermediate is held in int64 and asserted to fit int32."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_enc")
# name -> (H, W, channels, quality, subsampling): the fixtures of tests/golden/make_jpeg_encode_golden.py
CASES = {
    "rgb_1x1": (1, 1, 3, 95, "4:2:0"),
    "rgb_3x5": (3, 5, 3, 95, "4:2:0"),
    "rgb_8x24": (8, 24, 3, 95, "4:2:0"),
    "rgb_17x33": (17, 33, 3, 95, "4:2:0"),
    "noise_q30_24x40": (24, 40, 3, 30, "4:2:0"),
    "noise_q100_16x24": (16, 24, 3, 100, "4:2:0"),
    "rgb_q1_9x4": (9, 4, 3, 1, "4:2:0"),
    "s444_19x21": (19, 21, 3, 95, "4:4:4"),
    "s422_17x35": (17, 35, 3, 95, "4:2:2"),
    "grey_9x11": (9, 11, 1, 95, "4:2:0"),
    "mask_37x43": (37, 43, 1, 95, "4:2:0"),
    "ramp_q85_97x130": (97, 130, 3, 85, "4:2:0"),
}
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}  # luma (h, v); chroma is 1x1

LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K.3 - K.6: (counts of codes of length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def pixels(name):
    return np.load(os.path.join(GOLDEN, name + ".npy"))


def stream(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def decoded(name):
    """what Pillow decodes from ``stream(name)``: uint8 [H,W,3] or [H,W]"""
    return np.load(os.path.join(GOLDEN, name + ".dec.npy"))


def _i32(x):
    assert np.all(np.abs(x) < (1 << 31)), "an intermediate leaves int32"
    return x


def quant_tables(quality):
    """-> uint8 [2, 64]: the luminance and the chrominance table in natural order"""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (LUMA_Q, CHROMA_Q)], np.uint8)


def ceil_div(a, b):
    return -(-a // b)


def grids(H, W, C, hmax, vmax):
    """-> per component ((blocks_h, blocks_w) padded to whole MCUs, (real_h, real_w), (h, v))"""
    out = []
    for c in range(C):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        padded = (ceil_div(H, 8 * vmax) * v, ceil_div(W, 8 * hmax) * h)
        real = (ceil_div(ceil_div(H * v, vmax), 8), ceil_div(ceil_div(W * h, hmax), 8))
        out.append((padded, real, (h, v)))
    return out


def colour(rgb):
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    y = _i32(19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = _i32(-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = _i32(32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def component_plane(src, fx, fy, rows, cols):
    """One full-resolution component [H, W] -> its [rows, cols] sample plane (the real block grid times 8) by the edge rules: source
    columns replicated out to the padded width, source rows to a whole row group, then the downsampled rows replicated downwards."""
    H, W = src.shape
    src = src[:, np.minimum(np.arange(cols * fx), W - 1)]  # to the right: the source
    Hg = ceil_div(H, fy) * fy
    src = src[np.minimum(np.arange(Hg), H - 1)]  # downwards: the source to a whole row group only
    if fx == 2 and fy == 2:
        bias = np.tile([1, 2], cols)[:cols]
        p = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + bias) >> 2
    elif fx == 2:
        bias = np.tile([0, 1], cols)[:cols]
        p = (src[:, 0::2] + src[:, 1::2] + bias) >> 1
    else:
        assert fx == 1 and fy == 1
        p = src
    return p[np.minimum(np.arange(rows), p.shape[0] - 1)]  # then the last downsampled row


def _fdct8(d, first):
    """jfdctint.c's 1-D kernel along the last axis of int64 [..., 8]"""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 11 if first else 15
    ds = lambda x: (_i32(x) + (1 << (sh - 1))) >> sh  # noqa: E731
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = _i32((t12 + t13) * 4433)
    out[2] = ds(z1 + t13 * 6270)
    out[6] = ds(z1 - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = _i32((z3 + z4) * 9633)
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = ds(t4 + z1 + z3), ds(t5 + z2 + z4), ds(t6 + z2 + z3), ds(t7 + z1 + z4)
    return _i32(np.stack(out, axis=-1))


def fdct_quant(plane, q):
    """uint8-valued [8 * bh, 8 * bw] plane, natural-order table [64] -> int64 [bh, bw, 64]"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    rows = _fdct8(blocks, True)
    cols = _fdct8(rows.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    c = cols.reshape(bh, bw, 64)
    div = 8 * q.astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (div >> 1)) // div)


def layout(shapes, subsampling="4:2:0"):
    """[(H, W, C)] -> ([per image: [(coef offset, padded grid, real grid, (h, v)) per component], (hmax, vmax)], total coefficients)"""
    out, pos = [], 0
    for H, W, C in shapes:
        hmax, vmax = SAMPLING[subsampling] if C == 3 else (1, 1)
        comps = []
        for padded, real, hv in grids(H, W, C, hmax, vmax):
            comps.append((pos, padded, real, hv))
            pos += 64 * padded[0] * padded[1]
        out.append((comps, (hmax, vmax)))
    return out, pos


def forward_image(img, quality, subsampling, comps, hmax, vmax, coef):
    img = np.asarray(img)
    C = 1 if img.ndim == 2 else img.shape[2]
    q = quant_tables(quality)
    planes = colour(img) if C == 3 else [img.astype(np.int64)]
    for c, (off, (ph, pw), (rh, rw), (h, v)) in enumerate(comps):
        real = fdct_quant(component_plane(planes[c], hmax // h, vmax // v, 8 * rh, 8 * rw), q[min(c, 1)])
        full = np.zeros((ph, pw, 64), np.int64)
        full[:rh, :rw] = real
        for by in range(ph):  # dummy blocks: DC of the previous block of the MCU, in MCU order
            for bx in range(pw):
                if by >= rh:
                    sy, sx = rh - 1, min(bx // h * h + h - 1, rw - 1)
                elif bx >= rw:
                    sy, sx = by, rw - 1
                else:
                    continue
                full[by, bx, 0] = real[sy, sx, 0]
        coef[off:off + 64 * ph * pw] = full.reshape(-1)


def forward(images, quality=95, subsampling="4:2:0"):
    """list of uint8 [H,W,3] / [H,W] -> (coef int16 [n], layout): the coefficient buffer in the decoder's layout, dummy blocks included"""
    shapes = [(im.shape[0], im.shape[1], 1 if im.ndim == 2 else im.shape[2]) for im in images]
    lay, n = layout(shapes, subsampling)
    coef = np.zeros(n, np.int16)
    for im, (comps, (hmax, vmax)) in zip(images, lay):
        forward_image(im, quality, subsampling, comps, hmax, vmax, coef)
    return coef, lay


def _codes(spec):
    counts, vals = spec
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def header(H, W, C, hmax, vmax, q, density=(300, 300, "in")):
    units = {"in": 1, "cm": 2, None: 0, "": 0}[density[2]]
    out = b"\xFF\xD8" + _segment(0xE0, b"JFIF\0\x01\x01" + bytes([units]) + int(density[0]).to_bytes(2, "big") + int(density[1]).to_bytes(2, "big") + b"\0\0")
    for t in range(2 if C == 3 else 1):
        out += _segment(0xDB, bytes([t]) + bytes(int(q[t][ZIGZAG[i]]) for i in range(64)))
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([C])
    for c in range(C):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        sof += bytes([c + 1, h << 4 | v, min(c, 1)])
    out += _segment(0xC0, sof)
    for tc_th, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))[:4 if C == 3 else 2]:
        out += _segment(0xC4, bytes([tc_th]) + bytes(spec[0]) + bytes(spec[1]))
    sos = bytes([C]) + b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in range(C)) + b"\x00\x3F\x00"
    return out + _segment(0xDA, sos)


def entropy(coef, comps, hmax, vmax):
    """the scan's bytes (stuffed, padded with 1-bits) of one image's coefficient planes"""
    dc = [_codes(DC_LUMA), _codes(DC_CHROMA)]
    ac = [_codes(AC_LUMA), _codes(AC_CHROMA)]
    acc, nbits = 0, 0  # python ints: the whole scan as one number
    pred = [0] * len(comps)
    mcus_y, mcus_x = comps[0][1][0] // comps[0][3][1], comps[0][1][1] // comps[0][3][0]

    def put(code, length):
        nonlocal acc, nbits
        acc = (acc << length) | code
        nbits += length

    def magnitude(v):
        s = int(abs(v)).bit_length()
        return s, (v if v >= 0 else v + (1 << s) - 1)

    for my in range(mcus_y):
        for mx in range(mcus_x):
            for c, (off, (ph, pw), _, (h, v)) in enumerate(comps):
                for dy in range(v):
                    for dx in range(h):
                        o = off + 64 * ((my * v + dy) * pw + mx * h + dx)
                        blk = [int(x) for x in coef[o:o + 64]]
                        s, bits = magnitude(blk[0] - pred[c])
                        pred[c] = blk[0]
                        put(*dc[min(c, 1)][s])
                        if s:
                            put(bits, s)
                        run = 0
                        for k in range(1, 64):
                            x = blk[ZIGZAG[k]]
                            if x == 0:
                                run += 1
                                continue
                            while run > 15:
                                put(*ac[min(c, 1)][0xF0])
                                run -= 16
                            s, bits = magnitude(x)
                            put(*ac[min(c, 1)][run << 4 | s])
                            put(bits, s)
                            run = 0
                        if run:
                            put(*ac[min(c, 1)][0x00])
    pad = -nbits % 8
    put((1 << pad) - 1, pad)
    raw = acc.to_bytes(nbits // 8, "big")
    return raw.replace(b"\xFF", b"\xFF\x00")


def encode(img, quality=95, subsampling="4:2:0", density=(300, 300, "in")):
    """one frame -> the whole stream"""
    img = np.asarray(img)
    coef, lay = forward([img], quality, subsampling)
    comps, (hmax, vmax) = lay[0]
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else 3
    return header(H, W, C, hmax, vmax, quant_tables(quality), density) + entropy(coef, comps, hmax, vmax) + b"\xFF\xD9"
