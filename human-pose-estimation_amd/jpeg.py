"""JPEG decode for the training records: ``tf.image.decode_jpeg(buf, channels)`` (src/util/data_utils.py:129-141) for a whole batch.
Entropy decoding runs on the host (hpe_jpeg_decode, csrc/jpeg_entropy.hip: a pool of threads over the images); dequantisation, inverse
DCT, chroma upsampling, colour conversion and the store are two launches (hpe_jpeg_backend, csrc/jpeg_decode.hip).  The result is
libjpeg's default decode bit for bit; what is accepted and what is computed is defined in DESIGN.md "Training records and JPEG decode".
HIP-backed through include/hpe.h; no CPU fallback and no image library."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

# HpeJpegInfo / HpeJpegImage (include/hpe.h) as numpy records
INFO_DTYPE = np.dtype([("status", "<i4"), ("H", "<i4"), ("W", "<i4"), ("ncomp", "<i4"), ("hs", "<i4", 3), ("vs", "<i4", 3),
                       ("blocks_w", "<i4", 3), ("blocks_h", "<i4", 3), ("coefs", "<i8")])
TABLE_DTYPE = np.dtype([("coef_offset", "<i8", 3), ("plane_offset", "<i8", 3), ("out_offset", "<i8"), ("H", "<i4"), ("W", "<i4"),
                        ("ncomp", "<i4"), ("channels", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"), ("blocks_w", "<i4", 3),
                        ("blocks_h", "<i4", 3), ("idct_group0", "<i4"), ("store_group0", "<i4"), ("quant", "u1", (3, 64))])
assert INFO_DTYPE.itemsize == C.sizeof(_lib.HpeJpegInfo) == 72
assert TABLE_DTYPE.itemsize == C.sizeof(_lib.HpeJpegImage) == 304
DEFAULT_THREADS = 8  # a plain argument everywhere; never derived from the machine's core count

_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _stream_args(streams):
    """-> (arrays kept alive, pointer array, lengths int64 [B]) of a list of bytes-like JPEG streams"""
    if isinstance(streams, (bytes, bytearray, memoryview)) or not hasattr(streams, "__len__"):
        raise ValueError("streams must be a list of bytes objects")
    if len(streams) < 1:
        raise ValueError("streams is empty")
    keep = []
    for s in streams:
        if not isinstance(s, (bytes, bytearray, memoryview, np.ndarray)):
            raise ValueError("every stream must be bytes-like")
        keep.append(np.frombuffer(s.tobytes() if isinstance(s, np.ndarray) else bytes(s), dtype=np.uint8))
    lengths = np.array([a.size for a in keep], np.int64)
    keep = [a if a.size else np.zeros(1, np.uint8) for a in keep]  # an empty stream still needs an address; its length stays 0
    ptrs = (C.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
    return keep, ptrs, lengths


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


class DecodedBatch:
    """Decoded frames in one device buffer, each on a 16-byte boundary (the packing ``augment_batch`` uses): ``buffer`` uint8 CUDA
    tensor, ``sizes`` int64 [B,2] (H, W), ``offsets`` int64 [B] (bytes), ``channels`` 1 or 3, ``frames`` a list of views [H,W,3] (or
    [H,W] for one channel)."""

    def __init__(self, buffer, sizes, offsets, channels):
        self.buffer, self.sizes, self.offsets, self.channels = buffer, sizes, offsets, int(channels)

    def __len__(self):
        return int(self.sizes.shape[0])

    @property
    def frames(self):
        out = []
        for (h, w), o in zip(self.sizes.tolist(), self.offsets.tolist()):
            v = self.buffer[o:o + h * w * self.channels]
            out.append(v.view(h, w, 3) if self.channels == 3 else v.view(h, w))
        return out


def decode_jpeg_batch(streams, channels=3, threads=DEFAULT_THREADS, out=None):
    """``tf.image.decode_jpeg(s, channels=channels)`` of every stream -> ``DecodedBatch`` on the current CUDA device.  channels is 1 or
    3 for the whole batch.  The coefficients and the table are written into ONE pinned buffer, go up in one non-blocking copy, and the
    two back-end launches follow on the current stream; nothing reads the device.  A refused stream raises HpeError naming its index
    before anything is launched.  out: an optional contiguous uint8 CUDA tensor to decode into (at least the packed size; bytes
    between and after the frames are left as they are)."""
    import torch

    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    dev = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    if out is not None and (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or
                            not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 1-D uint8 CUDA tensor on a 16-byte boundary")
    pinned = []

    def alloc(n, B):
        buf = torch.empty(2 * n + B * TABLE_DTYPE.itemsize, dtype=torch.uint8, pin_memory=True)
        pinned.append(buf)
        host = buf.numpy()
        return host[:2 * n].view(np.int16), host[2 * n:].view(TABLE_DTYPE)

    with torch.cuda.device(dev):
        coef, table, totals = entropy_decode(streams, channels, threads, alloc)
        n, B = coef.shape[0], table.shape[0]
        need = int(totals[2])
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=dev)
        elif out.numel() < need:
            raise ValueError("out holds %d bytes, the packed frames need %d" % (out.numel(), need))
        staged = torch.empty(pinned[0].numel(), dtype=torch.uint8, device=dev)
        staged.copy_(pinned[0], non_blocking=True)
        workspace = torch.empty(int(totals[1]), dtype=torch.uint8, device=dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().hpe_jpeg_backend(_p(table), staged.data_ptr() + 2 * n, B, staged.data_ptr(), n, workspace.data_ptr(),
                                                workspace.numel(), out.data_ptr(), out.numel(), st))
    sizes = np.stack([table["H"], table["W"]], axis=1).astype(np.int64)
    return DecodedBatch(out, sizes, table["out_offset"].astype(np.int64), channels)
