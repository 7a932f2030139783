"""What the image codecs (jpeg, png, png_encode, jpeg_encode, augment, draw) share between their formats and their launches: argument
checks, the 16-byte packing of a batch of frames, ``DecodedBatch``, and the staging through pinned memory on the current stream.
Imports nothing from the codec modules; DESIGN.md "Codec plumbing"."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import HpeError

DEFAULT_THREADS = 8  # a plain argument everywhere; never derived from the machine's core count
MAX_SIDE = 16384  # of a frame to encode: HPE_PNG_MAX_SIDE and HPE_JPEG_MAX_SIDE

ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
up16 = lambda n: (int(n) + 15) // 16 * 16  # noqa: E731


def thread_count(threads, error=ValueError):
    """-> int(threads), or ``error``: ValueError keeps the decoders' text, any other type names the value as the JPEG encoder does"""
    if int(threads) != threads or not 1 <= int(threads) <= 16:
        raise error("threads must be an integer in [1, 16]" + ("" if error is ValueError else ", got %r" % (threads,)))
    return int(threads)


def stream_list(streams):
    """a list of bytes-like streams -> (list of bytes, lengths int64 [B]).  An empty stream is a one-byte stand-in, so that it still has
    an address; its length stays 0."""
    if isinstance(streams, (bytes, bytearray, memoryview)) or not hasattr(streams, "__len__"):
        raise ValueError("streams must be a list of bytes objects")
    if len(streams) < 1:
        raise ValueError("streams is empty")
    out = []
    for s in streams:
        if not isinstance(s, (bytes, bytearray, memoryview, np.ndarray)):
            raise ValueError("every stream must be bytes-like")
        out.append(s.tobytes() if isinstance(s, np.ndarray) else bytes(s))
    return [s or b"\0" for s in out], np.array([len(s) for s in out], np.int64)


def frame_offsets(sizes, channels):
    """sizes [B,2] (H, W) -> (byte offsets [B] of frames packed in order, each on a 16-byte boundary; total bytes): DecodedBatch's packing"""
    offs, pos = [], 0
    for h, w in np.asarray(sizes).reshape(-1, 2).tolist():
        offs.append(pos)
        pos += up16(h * w * channels)
    return np.array(offs, np.int64), pos


class DecodedBatch:
    """Decoded frames in one device buffer, each on a 16-byte boundary (the packing ``augment_batch`` uses): ``buffer`` uint8 CUDA
    tensor, ``sizes`` int64 [B,2] (H, W), ``offsets`` int64 [B] (bytes), ``channels`` 1 or 3, ``frames`` a list of views [H,W,3] (or
    [H,W] for one channel), ``nbytes`` the end of the last frame rounded up to 16."""

    def __init__(self, buffer, sizes, offsets, channels):
        self.buffer, self.sizes, self.offsets, self.channels = buffer, sizes, offsets, int(channels)

    def __len__(self):
        return int(self.sizes.shape[0])

    @property
    def nbytes(self):
        return int(self.offsets[-1]) + up16(int(self.sizes[-1, 0]) * int(self.sizes[-1, 1]) * self.channels)

    @property
    def frames(self):
        out = []
        for (h, w), o in zip(self.sizes.tolist(), self.offsets.tolist()):
            v = self.buffer[o:o + h * w * self.channels]
            out.append(v.view(h, w, 3) if self.channels == 3 else v.view(h, w))
        return out


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


def pack_frames(frames, channels):
    """The frames of an encoder -> (1-D uint8 CUDA buffer, [(H, W, C)], frame byte offsets): a [B,H,W,C] / [B,H,W] tensor and a
    ``DecodedBatch`` are used as they lie, a list of [H,W,C] / [H,W] tensors is packed with every frame on a 16-byte boundary.
    ``channels``: the channel counts the encoder takes, any container.  Raises HpeError naming the image and the clause."""
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
            if up16(n) > n:
                parts.append(torch.zeros(up16(n) - n, dtype=torch.uint8, device=t.device))
            pos += up16(n)
        buf = None
    else:
        raise ValueError("frames must be a CUDA uint8 tensor [B,H,W,C] or [B,H,W], a list of [H,W,C] / [H,W] tensors, or a DecodedBatch")
    for i, (H, W, Cn) in enumerate(shapes):
        if Cn not in channels:
            allowed = sorted(channels)
            raise HpeError("image %d: %d channels: the channel count must be %s or %d" % (i, Cn, ", ".join(map(str, allowed[:-1])), allowed[-1]))
        if H < 1 or W < 1:
            raise HpeError("image %d: an empty side: %d x %d (H x W)" % (i, H, W))
        if H > MAX_SIDE or W > MAX_SIDE:
            raise HpeError("image %d: a side of %d x %d (H x W) is above %d" % (i, H, W, MAX_SIDE))
    if buf is None:
        buf = torch.cat(parts) if len(parts) > 1 else parts[0]
    return buf, shapes, offsets


def check_out(out):
    """the ``out`` of a decoder, None or a packed-frame buffer -> the device to decode on"""
    import torch

    if out is not None and (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 1 or
                            not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 1-D uint8 CUDA tensor on a 16-byte boundary")
    return out.device if out is not None else torch.device("cuda", torch.cuda.current_device())


def frames_out(out, need, dev):
    """``out`` when it holds the ``need`` packed bytes, a new buffer when it is None"""
    import torch

    if out is None:
        return torch.empty(need, dtype=torch.uint8, device=dev)
    if out.numel() < need:
        raise ValueError("out holds %d bytes, the packed frames need %d" % (out.numel(), need))
    return out


def pinned(nbytes):
    """-> (pinned uint8 tensor [nbytes], its numpy view)"""
    import torch

    t = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    return t, t.numpy()


def upload(pinned_t, dev):
    """a pinned tensor -> a new device tensor, by one non-blocking copy on the current stream"""
    import torch

    t = torch.empty(pinned_t.numel(), dtype=pinned_t.dtype, device=dev)
    t.copy_(pinned_t, non_blocking=True)
    return t


def upload_table(table, dev):
    """a host record array -> its bytes on the device, through pinned memory"""
    p, view = pinned(table.nbytes)
    view[:] = table.view(np.uint8)
    return upload(p, dev)


def download(tensor):
    """a device tensor -> numpy, through pinned memory; waits for the current stream of the tensor's device"""
    import torch

    with torch.cuda.device(tensor.device):
        host = torch.empty(tensor.numel(), dtype=tensor.dtype, pin_memory=True)
        host.copy_(tensor, non_blocking=True)
        torch.cuda.current_stream(tensor.device).synchronize()
    return host.numpy()


def stream_ptr(dev):
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
