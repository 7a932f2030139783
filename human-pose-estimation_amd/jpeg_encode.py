"""JPEG encode for the dataset writers, the mirror of jpeg.py: ``tf.image.encode_jpeg`` (src/util/create_dataset.py:36-40) for a whole
batch of frames that are already on the device.  Everything per sample -- colour conversion, chroma downsampling, forward DCT and
quantisation -- is ONE launch (hpe_jpeg_forward, csrc/jpeg_encode.hip); the coefficients come down in one copy to pinned memory and
the serial entropy coder runs on host threads (hpe_jpeg_entropy_encode, csrc/jpeg_huffman_enc.hip).  The result is libjpeg's default
baseline compressor byte for byte; what is computed is defined in DESIGN.md "Dataset writers and JPEG encode".  HIP-backed through
include/hpe.h; no CPU fallback and no image library."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import HpeError
from .batch_io import DEFAULT_THREADS, download, pack_frames, ptr as _p, stream_ptr, thread_count, upload_table

# HpeJpegEncImage (include/hpe.h) as a numpy record
ENC_DTYPE = _lib.record_dtype(_lib.HpeJpegEncImage)
CHANNELS = (1, 3)  # grey, RGB
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}  # luma (h, v); chroma is 1x1
UNITS = {None: 0, "": 0, "none": 0, "in": 1, "cm": 2}
DEFAULT_DENSITY = (300, 300, "in")


def _quality(quality):
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise HpeError("quality must be an integer in [1, 100], got %r" % (quality,))
    return q


def _sampling(subsampling):
    if subsampling not in SAMPLING:
        raise HpeError("subsampling must be one of '4:4:4', '4:2:2', '4:2:0', got %r" % (subsampling,))
    return SAMPLING[subsampling]


def _density(density):
    try:
        x, y, unit = density
        x, y, unit = int(x), int(y), UNITS[unit]
    except (TypeError, ValueError, KeyError):
        raise HpeError("density must be (x, y, 'in' | 'cm' | None), got %r" % (density,)) from None
    if not (1 <= x <= 65535 and 1 <= y <= 65535):
        raise HpeError("density: x and y must be in [1, 65535]")
    return x, y, unit


def encode_layout(shapes, offsets=None, quality=95, subsampling="4:2:0"):
    """hpe_jpeg_encode_layout: [(H, W, C)] and the frames' byte offsets (default: packed back to back) -> (table record array [B] of
    ``ENC_DTYPE``, totals int64 [3] = coefficients, workgroups, stream-buffer bound).  Pure host code."""
    quality, (hmax, vmax) = _quality(quality), _sampling(subsampling)
    sh = np.ascontiguousarray(shapes, dtype=np.int32).reshape(-1, 3)
    if offsets is None:
        sizes = sh[:, 0].astype(np.int64) * sh[:, 1] * sh[:, 2]
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    if len(sh) < 1 or off.shape != (len(sh),):
        raise ValueError("shapes must be a non-empty list of (H, W, C) with one offset each")
    table = np.zeros(len(sh), ENC_DTYPE)
    totals = np.zeros(3, np.int64)
    _lib.check(_lib.load().hpe_jpeg_encode_layout(len(sh), _p(sh), _p(off), hmax, vmax, quality, _p(table), _p(totals)))
    return table, totals


def quant_tables(quality):
    """-> uint8 [2, 64]: the luminance and chrominance quantisation tables of ``quality`` (1 .. 100) in natural order"""
    table, _ = encode_layout([(8, 8, 3)], quality=quality)
    return table[0]["quant"].copy()


def entropy_encode(coef, table, density=DEFAULT_DENSITY, threads=DEFAULT_THREADS, out=None):
    """The host half alone (hpe_jpeg_entropy_encode): host coefficients int16 [n] and their table -> list[bytes] of whole streams.
    ``out``: an optional uint8 array to write into, at least the bound ``sum(stream_bound(table))`` long (smaller is refused before
    anything is written).  The bytes do not depend on ``threads`` (1 .. 16)."""
    x, y, unit = _density(density)
    threads = thread_count(threads, HpeError)
    coef = np.ascontiguousarray(coef, dtype=np.int16)
    table = np.ascontiguousarray(table, dtype=ENC_DTYPE)
    B = len(table)
    if out is None:
        out = np.empty(int(stream_bound(table).sum()), np.uint8)
    if out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
        raise ValueError("out must be a contiguous 1-D uint8 array")
    offsets, lengths = np.zeros(B, np.int64), np.zeros(B, np.int64)
    _lib.check(_lib.load().hpe_jpeg_entropy_encode(_p(table), B, _p(coef), coef.size, unit, x, y, int(threads), _p(out), out.size, _p(offsets),
                                                   _p(lengths)))
    return [out[o:o + n].tobytes() for o, n in zip(offsets.tolist(), lengths.tolist())]


def stream_bound(table):
    """-> int64 [B]: the documented bound of every image's stream, HPE_JPEG_ENC_HEADER_BYTES + HPE_JPEG_ENC_BLOCK_BYTES * blocks"""
    t = np.atleast_1d(table)
    blocks = (t["blocks_w"].astype(np.int64) * t["blocks_h"]).sum(axis=1)
    return 640 + 416 * blocks


def table_from_decoded(table):
    """``jpeg.TABLE_DTYPE`` entries of ``entropy_decode`` -> ``ENC_DTYPE`` entries over the SAME coefficient buffer, so that what was
    decoded can be coded again: sizes, sampling, grids and offsets are kept, quantisation tables 0 and 1 are the stream's luminance and
    first chrominance table.  The frame offsets are 0: these entries are for ``entropy_encode``, not for the launch."""
    src = np.atleast_1d(table)
    out = np.zeros(len(src), ENC_DTYPE)
    group = 0
    for e, d in zip(src, out):
        n, hmax, vmax = int(e["ncomp"]), int(e["hmax"]), int(e["vmax"])
        if n == 1:
            hmax = vmax = 1  # Y alone: a grey stream of its own
        d["H"], d["W"], d["C"], d["hmax"], d["vmax"], d["group0"] = e["H"], e["W"], n, hmax, vmax, group
        for c in range(n):
            h, v = (hmax, vmax) if c == 0 else (1, 1)
            d["coef_offset"][c], d["blocks_w"][c], d["blocks_h"][c] = e["coef_offset"][c], e["blocks_w"][c], e["blocks_h"][c]
            d["real_w"][c] = -(-(-(-int(e["W"]) * h // hmax)) // 8)
            d["real_h"][c] = -(-(-(-int(e["H"]) * v // vmax)) // 8)
        d["quant"][0], d["quant"][1] = e["quant"][0], e["quant"][1 if n == 3 else 0]
        group += -(-int((d["blocks_w"].astype(np.int64) * d["blocks_h"]).sum()) // 32)
    return out


def forward_dct_batch(frames, quality=95, subsampling="4:2:0", out=None):
    """The device half alone: -> (coef int16 CUDA [n], table).  The coefficient buffer has the decoder's layout (jpeg.TABLE_DTYPE's
    coef_offset / blocks_w / blocks_h), dummy blocks included.  One launch on the current stream; nothing reads the device.  ``out``:
    an optional contiguous int16 CUDA tensor to write into; elements outside the images' planes are left as they are."""
    import torch

    quality, _ = _quality(quality), _sampling(subsampling)
    buf, shapes, offsets = pack_frames(frames, CHANNELS)
    table, totals = encode_layout(shapes, offsets, quality, subsampling)
    n, dev = int(totals[0]), buf.device
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.int16 or out.dim() != 1 or
                            not out.is_contiguous() or out.data_ptr() % 16 or out.numel() < n):
        raise ValueError("out must be a contiguous 1-D int16 tensor on the frames' device, on a 16-byte boundary, of at least %d elements" % n)
    with torch.cuda.device(dev):
        table_dev = upload_table(table, dev)
        coef = torch.empty(n, dtype=torch.int16, device=dev) if out is None else out
        _lib.check(_lib.load().hpe_jpeg_forward(_p(table), table_dev.data_ptr(), len(shapes), buf.data_ptr(), buf.numel(), coef.data_ptr(),
                                                coef.numel(), stream_ptr(dev)))
    return coef, table


def encode_jpeg_batch(frames, quality=95, subsampling="4:2:0", density=DEFAULT_DENSITY, threads=DEFAULT_THREADS):
    """Every frame as a baseline JPEG stream -> list[bytes], what ``tf.image.encode_jpeg`` / Pillow's ``save(..., quality=quality,
    subsampling=subsampling, dpi=density[:2])`` write.  frames: a CUDA uint8 tensor [B,H,W,C] or [B,H,W], a list of [H,W,C] / [H,W]
    tensors of different sizes, or a ``DecodedBatch``; C is 1 (grey) or 3 (RGB), sides are 1 .. 16384; ``subsampling`` is ignored for
    grey frames.  Anything else raises HpeError naming the image and the clause, before anything is launched.  The table goes up in one
    pinned copy, one launch computes every coefficient, they come down in one copy, and the Huffman coder runs per image on ``threads``
    host threads (1 .. 16).  The bytes do not depend on ``threads``.  This call waits for the device."""
    _density(density)
    threads = thread_count(threads, HpeError)
    coef, table = forward_dct_batch(frames, quality, subsampling)
    return entropy_encode(download(coef), table, density, threads)
