"""JPEG decode for the training records: ``tf.image.decode_jpeg(buf, channels)`` (src/util/data_utils.py:129-141) for a whole batch.
Entropy decoding runs on the host (hpe_jpeg_decode, csrc/jpeg_entropy.hip: a pool of threads over the images); dequantisation, inverse
DCT, chroma upsampling, colour conversion and the store are two launches (hpe_jpeg_backend, csrc/jpeg_decode.hip).  The result is
libjpeg's default decode bit for bit; what is accepted and what is computed is defined in DESIGN.md "Training records and JPEG decode".
HIP-backed through include/hpe.h; no CPU fallback and no image library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .batch_io import DEFAULT_THREADS, DecodedBatch, check_out, frames_out, pinned, ptr as _p, stream_list, stream_ptr, upload

# HpeJpegInfo / HpeJpegImage (include/hpe.h) as numpy records
INFO_DTYPE = _lib.record_dtype(_lib.HpeJpegInfo)
TABLE_DTYPE = _lib.record_dtype(_lib.HpeJpegImage)


def _stream_args(streams):
    """-> (bytes kept alive, pointer array, lengths int64 [B]) of a list of bytes-like JPEG streams"""
    data, lengths = stream_list(streams)
    return data, (C.c_char_p * len(data))(*data), lengths


def _channels(channels, B):
    ch = np.full(B, channels, np.int32) if np.isscalar(channels) else np.ascontiguousarray(channels, dtype=np.int32)
    if ch.shape != (B,):
        raise ValueError("channels must be 1, 3 or one of them per stream")
    return ch


def jpeg_info(data):
    """hpe_jpeg_info of one stream: {'height', 'width', 'components', 'sampling' [(h, v)] per component, 'blocks' [(rows, columns)] of
    every component's block grid, 'coefficients'}.  A stream outside the accepted subset raises HpeError with the clause.  Pure host."""
    keep, ptrs, lengths = _stream_args([data])
    info = np.zeros(1, INFO_DTYPE)
    _lib.check(_lib.load().hpe_jpeg_info(1, ptrs, _p(lengths), _p(info)))
    i = info[0]
    n = int(i["ncomp"])
    return {"height": int(i["H"]), "width": int(i["W"]), "components": n, "sampling": [(int(i["hs"][c]), int(i["vs"][c])) for c in range(n)],
            "blocks": [(int(i["blocks_h"][c]), int(i["blocks_w"][c])) for c in range(n)], "coefficients": int(i["coefs"])}


def entropy_decode(streams, channels=3, threads=DEFAULT_THREADS, alloc=None):
    """The host half alone (hpe_jpeg_decode): -> (coef int16 [totals[0]], table record array [B] of ``TABLE_DTYPE``, totals int64 [5] =
    coefficients, workspace bytes, frame bytes, workgroups of launch one and two).  ``alloc(n_coef, B)`` may return the (coef, table)
    arrays to fill, e.g. views of pinned memory.  Any refused stream raises HpeError naming the image, before anything is decoded when
    its header is the reason.  Pure host code: no device is needed."""
    keep, ptrs, lengths = _stream_args(streams)
    B = len(keep)
    ch = _channels(channels, B)
    lib = _lib.load()
    status = np.zeros(B, np.int32)
    totals = np.zeros(5, np.int64)
    layout = np.zeros(B, TABLE_DTYPE)
    _lib.check(lib.hpe_jpeg_decode(B, ptrs, _p(lengths), _p(ch), int(threads), None, 0, _p(layout), _p(status), _p(totals)))
    n = int(totals[0])
    coef, table = alloc(n, B) if alloc is not None else (np.empty(n, np.int16), np.zeros(B, TABLE_DTYPE))
    if coef.dtype != np.int16 or coef.shape != (n,) or table.dtype != TABLE_DTYPE or table.shape != (B,) or \
            not coef.flags.c_contiguous or not table.flags.c_contiguous:
        raise ValueError("alloc must return a contiguous int16 [n] array and a TABLE_DTYPE [B] array")
    _lib.check(lib.hpe_jpeg_decode(B, ptrs, _p(lengths), _p(ch), int(threads), _p(coef), n, _p(table), _p(status), _p(totals)))
    return coef, table, totals


def _pinned_alloc(keep):
    """``entropy_decode``'s alloc over ONE pinned buffer, coefficients then table; the buffer is appended to ``keep``"""
    def alloc(n, B):
        buf, host = pinned(2 * n + B * TABLE_DTYPE.itemsize)
        keep.append(buf)
        return host[:2 * n].view(np.int16), host[2 * n:].view(TABLE_DTYPE)

    return alloc


def _launch_jpeg(pinned_buf, table, totals, out, dev):
    """one non-blocking copy of the staged buffer and the two launches on the current stream"""
    import torch

    n = int(totals[0])
    staged = upload(pinned_buf, dev)
    workspace = torch.empty(int(totals[1]), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().hpe_jpeg_backend(_p(table), staged.data_ptr() + 2 * n, table.shape[0], staged.data_ptr(), n, workspace.data_ptr(),
                                            workspace.numel(), out.data_ptr(), out.numel(), stream_ptr(dev)))


def decode_jpeg_batch(streams, channels=3, threads=DEFAULT_THREADS, out=None):
    """``tf.image.decode_jpeg(s, channels=channels)`` of every stream -> ``DecodedBatch`` on the current CUDA device.  channels is 1 or
    3 for the whole batch.  The coefficients and the table are written into ONE pinned buffer, go up in one non-blocking copy, and the
    two back-end launches follow on the current stream; nothing reads the device.  A refused stream raises HpeError naming its index
    before anything is launched.  out: an optional contiguous uint8 CUDA tensor to decode into (at least the packed size; bytes
    between and after the frames are left as they are)."""
    import torch

    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    dev = check_out(out)
    keep = []
    with torch.cuda.device(dev):
        _, table, totals = entropy_decode(streams, channels, threads, _pinned_alloc(keep))
        out = frames_out(out, int(totals[2]), dev)
        _launch_jpeg(keep[0], table, totals, out, dev)
    sizes = np.stack([table["H"], table["W"]], axis=1).astype(np.int64)
    return DecodedBatch(out, sizes, table["out_offset"].astype(np.int64), channels)
