"""NumPy restatement of the PNG encoder (DESIGN.md "Training summaries"): the five filters, libpng's minimum-sum choice per row, and
the chunk wrapping.  It shares no code with csrc/png_encode.hip or hpe_amd/png_encode.py.  ``cases()`` are the frames the CPU and the
GPU tests share: the issue's shapes with content chosen so that every filter type is selected at least once."""
import struct
import zlib

import numpy as np

SHAPES = [(1, 1, 1), (1, 1, 3), (3, 1, 4), (1, 7, 3), (5, 7, 1), (17, 13, 3), (33, 65, 4), (9, 300, 1)]


def candidates(frame):
    """uint8 [H, W, C] -> uint8 [5, H, W*C]: every row under None, Sub, Up, Average, Paeth, from the raw neighbours with bpp = C; the
    row above the first and the bytes left of the first pixel are zero"""
    H, W, C = frame.shape
    rb = W * C
    x = frame.reshape(H, rb).astype(np.int64)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :rb - C]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :rb - C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))  # ties in the order a, b, c
    preds = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    return np.stack([(x - q) & 255 for q in preds]).astype(np.uint8)


def scores(cand):
    """[5, H, rb] -> int64 [5, H]: the sum over a row's bytes of v < 128 ? v : 256 - v"""
    v = cand.astype(np.int64)
    return np.where(v < 128, v, 256 - v).sum(axis=2)


def scanlines(frame):
    """uint8 [H, W, C] (or [H, W]) -> (uint8 [H, 1 + W*C], chosen filter types [H]): smallest score, then lowest filter number"""
    frame = frame if frame.ndim == 3 else frame[:, :, None]
    cand = candidates(frame)
    ft = np.argmin(scores(cand), axis=0)  # argmin returns the first of equal minima
    H = frame.shape[0]
    out = np.empty((H, 1 + cand.shape[2]), np.uint8)
    out[:, 0] = ft
    out[:, 1:] = cand[ft, np.arange(H)]
    return out, ft


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode(frame, level=6):
    """uint8 [H, W, C] or [H, W] -> the PNG stream: signature, IHDR, one IDAT, IEND"""
    frame = frame if frame.ndim == 3 else frame[:, :, None]
    H, W, C = frame.shape
    ihdr = struct.pack(">IIBBBBB", W, H, 8, {1: 0, 3: 2, 4: 6}[C], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(scanlines(frame)[0].tobytes(), level)) + _chunk(b"IEND", b"")


def content(H, W, C, seed):
    """ramps, noise, column-constant stripes and diagonals, in bands of rows, so that each filter has rows it wins: noise -> None,
    a horizontal ramp -> Sub, columns constant down the rows -> Up, a plane rising both ways -> Average / Paeth"""
    rng = np.random.RandomState(seed)
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    kinds = [
        rng.randint(0, 256, (H, W, C)),                       # noise
        (7 * x + 3 * c + 11 * (y // 4)) & 255,                # a ramp along the row, other rows unrelated
        np.broadcast_to(rng.randint(0, 256, (1, W, C)), (H, W, C)),  # column-constant stripes
        (5 * x + 9 * y + 40 * c) & 255,                       # a plane: x - (a + b - c) is 0
        (x * y + 3 * x + 2 * y) & 255,                        # a curved surface
        ((x + y) % 7 == 0) * 200 + rng.randint(0, 3, (H, W, C)),  # diagonals over faint noise
        np.zeros((H, W, C), np.int64),                        # all zero: the tie, filter 0
    ]
    band = (y + seed) // 3 % len(kinds) if H > 2 else (x // 2 + seed) % len(kinds)
    out = np.zeros((H, W, C), np.int64)
    for k, v in enumerate(kinds):
        out = np.where(band == k, v, out)
    return out.astype(np.uint8)


def cases():
    """[(name, uint8 [H, W, C])] for SHAPES"""
    return [("%dx%dx%d" % s, content(*s, seed=i)) for i, s in enumerate(SHAPES)]
