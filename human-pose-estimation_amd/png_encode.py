"""PNG encode for the training summaries, the mirror of png.py: frames that are already on the device become PNG streams.  Everything
per byte runs on the device -- the five PNG filters and libpng's minimum-sum choice per row are ONE launch over all rows of the batch
(hpe_png_filter, csrc/png_encode.hip) --, the serial part here on the host: the scanlines come down in one copy to pinned memory,
``zlib.compress`` runs per image on a pool of threads, and each result is wrapped in the signature, IHDR, one IDAT and IEND.  8-bit
samples, colour type 0, 2 or 6 by channel count, no interlace.  Lossless: ``decode_png_batch`` returns the frames bit for bit.
HIP-backed through include/hpe.h; no CPU fallback and no image library."""
from __future__ import annotations

import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from .batch_io import DEFAULT_THREADS, download, pack_frames, ptr as _p, stream_ptr, thread_count, up16, upload_table
from .png import SIGNATURE

COLOR_TYPE = {1: 0, 3: 2, 4: 6}  # channels -> IHDR colour type

# HpePngFilterImage (include/hpe.h) as a numpy record
FILTER_DTYPE = _lib.record_dtype(_lib.HpePngFilterImage)


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def wrap_png(H, W, channels, idat):
    """signature, IHDR (8-bit, colour type by channel count), one IDAT holding the zlib stream ``idat``, IEND"""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOR_TYPE[channels], 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def filter_table(shapes, offsets):
    """-> (table record array [B] of ``FILTER_DTYPE``, scanline bytes): every image's scanlines on a 16-byte boundary, in batch order"""
    table = np.zeros(len(shapes), FILTER_DTYPE)
    pos = rows = 0
    for b, ((H, W, Cn), o) in enumerate(zip(shapes, offsets)):
        table[b] = (o, pos, H, W, Cn, rows)
        pos += up16(H * (W * Cn + 1))
        rows += H
    return table, pos


def filter_batch(frames):
    """The device half alone: -> (scanlines uint8 CUDA [bytes], table).  Image b's H * (1 + W * C) scanline bytes start at
    ``table[b]['scan_offset']``.  One launch on the current stream; nothing reads the device."""
    import torch

    buf, shapes, offsets = pack_frames(frames, COLOR_TYPE)
    table, scan_bytes = filter_table(shapes, offsets)
    dev = buf.device
    with torch.cuda.device(dev):
        table_dev = upload_table(table, dev)
        scan = torch.zeros(scan_bytes, dtype=torch.uint8, device=dev)  # the padding between the images is defined too
        _lib.check(_lib.load().hpe_png_filter(_p(table), table_dev.data_ptr(), len(shapes), buf.data_ptr(), buf.numel(), scan.data_ptr(),
                                              scan.numel(), stream_ptr(dev)))
    return scan, table


def _level(level):
    lv = int(level)
    if lv != level or not -1 <= lv <= 9:
        raise ValueError("level must be an integer in [-1, 9]")
    return lv


def deflate_batch(scan_host, table, level=6, threads=DEFAULT_THREADS):
    """host scanlines (uint8 array) and their table -> list[bytes] of PNG streams; the bytes do not depend on ``threads``"""
    level, threads = _level(level), thread_count(threads)

    def one(e):
        o, H, W, Cn = int(e["scan_offset"]), int(e["H"]), int(e["W"]), int(e["C"])
        return wrap_png(H, W, Cn, zlib.compress(memoryview(scan_host[o:o + H * (W * Cn + 1)]), level))

    if threads == 1 or len(table) == 1:
        return [one(e) for e in table]
    with ThreadPoolExecutor(max_workers=min(threads, len(table))) as pool:
        return list(pool.map(one, table))


def encode_png_batch(frames, level=6, threads=DEFAULT_THREADS):
    """Every frame as a PNG stream -> list[bytes].  frames: a CUDA uint8 tensor [B,H,W,C] or [B,H,W], a list of [H,W,C] / [H,W]
    tensors of different sizes, or a ``DecodedBatch``; C is 1 (grey), 3 (RGB) or 4 (RGBA), sides are 1 .. 16384.  Anything else raises
    HpeError naming the image and the clause, before anything is launched.  The filter of every row is chosen on the device by
    libpng's minimum-sum rule (one launch for the whole batch); the scanlines come down in one copy, and ``zlib.compress(..., level)``
    runs per image on ``threads`` host threads (1 .. 16).  The bytes do not depend on ``threads``.  This call waits for the device."""
    level, threads = _level(level), thread_count(threads)
    scan, table = filter_batch(frames)
    return deflate_batch(download(scan), table, level, threads)
