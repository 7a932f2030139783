"""PNG encode for the training summaries, the mirror of png.py: frames that are already on the device become PNG streams.  Everything
per byte runs on the device -- the five PNG filters and libpng's minimum-sum choice per row are ONE launch over all rows of the batch
(hpe_png_filter, csrc/png_encode.hip) --, the serial part here on the host: the scanlines come down in one copy to pinned memory,
``zlib.compress`` runs per image on a pool of threads, and each result is wrapped in the signature, IHDR, one IDAT and IEND.  8-bit
samples, colour type 0, 2 or 6 by channel count, no interlace.  Lossless: ``decode_png_batch`` returns the frames bit for bit.
HIP-backed through include/hpe.h; no CPU fallback and no image library."""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from ._lib import HpeError
from .jpeg import DEFAULT_THREADS, DecodedBatch
from .png import MAX_SIDE, SIGNATURE, _p, _threads, _up16

COLOR_TYPE = {1: 0, 3: 2, 4: 6}  # channels -> IHDR colour type

# HpePngFilterImage (include/hpe.h) as a numpy record
FILTER_DTYPE = np.dtype([("frame_offset", "<i8"), ("scan_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("row0", "<i4")])
assert FILTER_DTYPE.itemsize == C.sizeof(_lib.HpePngFilterImage) == 32


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def wrap_png(H, W, channels, idat):
    """signature, IHDR (8-bit, colour type by channel count), one IDAT holding the zlib stream ``idat``, IEND"""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOR_TYPE[channels], 0, 0, 0)) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")


def _shape_fault(H, W, Cn):
    if Cn not in COLOR_TYPE:
        return "%d channels: the channel count must be 1, 3 or 4" % Cn
    if H < 1 or W < 1:
        return "an empty side: %d x %d (H x W)" % (H, W)
    if H > MAX_SIDE or W > MAX_SIDE:
        return "a side of %d x %d (H x W) is above %d" % (H, W, MAX_SIDE)
    return None


def _tensor_fault(t, dims):
    import torch

    if not isinstance(t, torch.Tensor):
        return "not a tensor but %s" % type(t).__name__
    if not t.is_cuda:
        return "the frame is not on a CUDA device"
    if t.dtype != torch.uint8:
        return "dtype %s: only uint8 frames are encoded" % str(t.dtype).replace("torch.", "")
    if t.dim() not in dims:
        return "a tensor of %d dimensions, not of %s" % (t.dim(), " or ".join(str(d) for d in dims))
    return None


def _layout(frames):
    """-> (1-D uint8 CUDA buffer, [(H, W, C)], frame byte offsets); raises HpeError naming the image and the clause"""
    import torch

    if isinstance(frames, DecodedBatch):
        shapes = [(int(h), int(w), frames.channels) for h, w in np.asarray(frames.sizes).reshape(-1, 2).tolist()]
        buf, offsets = frames.buffer, [int(o) for o in np.asarray(frames.offsets).reshape(-1).tolist()]
        fault = _tensor_fault(buf, (1,))
        if fault or not buf.is_contiguous():
            raise HpeError("image 0: the DecodedBatch's buffer: %s" % (fault or "not contiguous"))
    elif isinstance(frames, torch.Tensor):
        fault = _tensor_fault(frames, (3, 4))
        if fault:
            raise HpeError("image 0: %s" % fault)
        if frames.shape[0] < 1:
            raise ValueError("frames is empty")
        H, W = int(frames.shape[1]), int(frames.shape[2])
        Cn = int(frames.shape[3]) if frames.dim() == 4 else 1
        shapes = [(H, W, Cn)] * int(frames.shape[0])
        buf = frames.contiguous().reshape(-1)
        offsets = [b * H * W * Cn for b in range(len(shapes))]
    elif isinstance(frames, (list, tuple)):
        if len(frames) < 1:
            raise ValueError("frames is empty")
        shapes, offsets, parts, pos = [], [], [], 0
        for i, t in enumerate(frames):
            fault = _tensor_fault(t, (2, 3))
            if fault:
                raise HpeError("image %d: %s" % (i, fault))
            if t.device != frames[0].device:
                raise HpeError("image %d: the frame is on %s, image 0 on %s" % (i, t.device, frames[0].device))
            shapes.append((int(t.shape[0]), int(t.shape[1]), int(t.shape[2]) if t.dim() == 3 else 1))
            offsets.append(pos)
            n = t.numel()
            parts.append(t.contiguous().reshape(-1))
            if _up16(n) > n:
                parts.append(torch.zeros(_up16(n) - n, dtype=torch.uint8, device=t.device))
            pos += _up16(n)
        buf = None
    else:
        raise ValueError("frames must be a CUDA uint8 tensor [B,H,W,C] or [B,H,W], a list of [H,W,C] / [H,W] tensors, or a DecodedBatch")
    for i, (H, W, Cn) in enumerate(shapes):
        fault = _shape_fault(H, W, Cn)
        if fault:
            raise HpeError("image %d: %s" % (i, fault))
    if buf is None:
        buf = torch.cat(parts) if len(parts) > 1 else parts[0]
    return buf, shapes, offsets


def filter_table(shapes, offsets):
    """-> (table record array [B] of ``FILTER_DTYPE``, scanline bytes): every image's scanlines on a 16-byte boundary, in batch order"""
    table = np.zeros(len(shapes), FILTER_DTYPE)
    pos = rows = 0
    for b, ((H, W, Cn), o) in enumerate(zip(shapes, offsets)):
        table[b] = (o, pos, H, W, Cn, rows)
        pos += _up16(H * (W * Cn + 1))
        rows += H
    return table, pos


def filter_batch(frames):
    """The device half alone: -> (scanlines uint8 CUDA [bytes], table).  Image b's H * (1 + W * C) scanline bytes start at
    ``table[b]['scan_offset']``.  One launch on the current stream; nothing reads the device."""
    import torch

    buf, shapes, offsets = _layout(frames)
    table, scan_bytes = filter_table(shapes, offsets)
    dev = buf.device
    with torch.cuda.device(dev):
        pinned = torch.empty(table.nbytes, dtype=torch.uint8, pin_memory=True)
        pinned.numpy()[:] = table.view(np.uint8)
        table_dev = torch.empty(table.nbytes, dtype=torch.uint8, device=dev)
        table_dev.copy_(pinned, non_blocking=True)
        scan = torch.zeros(scan_bytes, dtype=torch.uint8, device=dev)  # the padding between the images is defined too
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().hpe_png_filter(_p(table), table_dev.data_ptr(), len(shapes), buf.data_ptr(), buf.numel(), scan.data_ptr(),
                                              scan.numel(), st))
    return scan, table


def _level(level):
    lv = int(level)
    if lv != level or not -1 <= lv <= 9:
        raise ValueError("level must be an integer in [-1, 9]")
    return lv


def deflate_batch(scan_host, table, level=6, threads=DEFAULT_THREADS):
    """host scanlines (uint8 array) and their table -> list[bytes] of PNG streams; the bytes do not depend on ``threads``"""
    level, threads = _level(level), _threads(threads)

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
    import torch

    level, threads = _level(level), _threads(threads)
    scan, table = filter_batch(frames)
    with torch.cuda.device(scan.device):
        host = torch.empty(scan.numel(), dtype=torch.uint8, pin_memory=True)
        host.copy_(scan, non_blocking=True)
        torch.cuda.current_stream(scan.device).synchronize()
    return deflate_batch(host.numpy(), table, level, threads)
