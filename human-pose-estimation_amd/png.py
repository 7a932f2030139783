"""PNG decode for the training records: the PNG streams ``tf.image.decode_jpeg(buf, channels)`` also takes (src/util/data_utils.py:129-141;
LSP masks are stored as PNG, MPII frames too), for a whole batch.  The serial part runs here on the host -- signature, chunk walk,
CRC-32, and inflate with the standard library's zlib on a pool of threads over the images -- and everything per byte on the device:
the PNG unfilter and the unpack / palette / channel conversion / store are two launches (hpe_png_backend, csrc/png_decode.hip).
Lossless, so the result is the encoded array bit for bit; what is accepted and refused is defined in DESIGN.md "PNG streams in the
records".  ``decode_image_batch`` takes JPEG and PNG streams side by side.  HIP-backed through include/hpe.h; no CPU fallback and no
image library."""
from __future__ import annotations

import re
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from ._lib import HpeError
from .batch_io import (DEFAULT_THREADS, DecodedBatch, check_out, frame_offsets, frames_out, pinned, ptr as _p, stream_list, stream_ptr,
                       thread_count, up16, upload)

SIGNATURE = b"\x89PNG\r\n\x1a\n"
JPEG_SOI = b"\xff\xd8"
MAX_SIDE = 16384
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}  # samples per pixel of every colour type
PALETTE_BYTES = 256 * 4  # on the device: 256 entries (R, G, B, 0), entries beyond PLTE zero
STORE_BYTES_PER_GROUP = 1024

# HpePngImage (include/hpe.h) as a numpy record
TABLE_DTYPE = _lib.record_dtype(_lib.HpePngImage)


class _Refused(Exception):
    """a clause without the image index: ``_named`` adds it"""


def _named(idx, e):
    return HpeError("image %d: %s" % (idx, e))


def is_direct(color_type, depth, channels):
    """8-bit grey asked for 1 channel, 8-bit RGB asked for 3: the unfiltered rows are the frame (png.h)"""
    return depth == 8 and ((color_type == 0 and channels == 1) or (color_type == 2 and channels == 3))


def _parse(data, verify=True):
    """Signature and chunk walk of one stream -> {'H', 'W', 'color_type', 'depth', 'samples', 'rowbytes', 'bpp', 'palette': bytes or None,
    'idat': [views of the IDAT bodies]}; raises _Refused with the clause."""
    n = len(data)
    data = memoryview(data)  # chunk bodies are views: nothing of the stream is copied before inflate
    if n < 8 or data[:8] != SIGNATURE:
        raise _Refused("not a PNG stream: the signature is missing")
    pos, hdr, palette, idat, idat_closed, ended = 8, None, None, [], False, False
    while pos < n:
        if n - pos < 12:
            raise _Refused("a chunk header is truncated at byte %d" % pos)
        length, kind = struct.unpack_from(">I4s", data, pos)
        if length > 0x7FFFFFFF or length > n - pos - 12:
            raise _Refused("chunk %r of %d bytes runs past the end of the stream" % (kind, length))
        body = data[pos + 8:pos + 8 + length]
        if verify and zlib.crc32(data[pos + 4:pos + 8 + length]) != struct.unpack_from(">I", data, pos + 8 + length)[0]:
            raise _Refused("bad CRC in chunk %r at byte %d" % (kind, pos))
        pos += 12 + length
        if hdr is None:
            if kind != b"IHDR" or length != 13:
                raise _Refused("the first chunk is not a 13-byte IHDR")
            W, H, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if W < 1 or H < 1 or W > MAX_SIDE or H > MAX_SIDE:
                raise _Refused("a side of %d x %d (W x H) is zero or above %d" % (W, H, MAX_SIDE))
            if ct not in SAMPLES:
                raise _Refused("colour type %d is not one of 0, 2, 3, 4, 6" % ct)
            if depth == 16 and ct != 3:
                raise _Refused("16-bit samples are not accepted")
            if depth not in (1, 2, 4, 8) or (depth != 8 and ct not in (0, 3)):
                raise _Refused("bit depth %d is not allowed for colour type %d" % (depth, ct))
            if comp != 0:
                raise _Refused("compression method %d is not 0" % comp)
            if filt != 0:
                raise _Refused("filter method %d is not 0" % filt)
            if lace == 1:
                raise _Refused("Adam7 interlace is not accepted")
            if lace != 0:
                raise _Refused("interlace method %d is not 0" % lace)
            samples = SAMPLES[ct]
            hdr = {"H": H, "W": W, "color_type": ct, "depth": depth, "samples": samples, "rowbytes": (W * samples * depth + 7) // 8,
                   "bpp": max(1, samples * depth // 8)}
            continue
        if kind == b"IDAT":
            if idat_closed:
                raise _Refused("the IDAT chunks are not consecutive")
            idat.append(body)
            continue
        if idat:
            idat_closed = True
        if kind == b"IEND":
            ended = True
            break
        if kind == b"IHDR":
            raise _Refused("IHDR is repeated")
        if kind == b"PLTE":
            if palette is not None:
                raise _Refused("PLTE is repeated")
            if idat:
                raise _Refused("PLTE follows IDAT")
            limit = 1 << hdr["depth"] if hdr["color_type"] == 3 else 256
            if length == 0 or length % 3 or length // 3 > limit:
                raise _Refused("an oversized or malformed PLTE: %d bytes, at most %d entries of 3" % (length, limit))
            palette = bytes(body)
            continue
        if not kind[0] & 0x20:  # an upper-case first letter: critical
            raise _Refused("unknown critical chunk %r" % kind)
        # ancillary (tRNS, gAMA, acTL, ...): skipped
    if hdr is None:
        raise _Refused("the stream ends before IHDR")
    if not ended:
        raise _Refused("the stream has no IEND")
    if not idat:
        raise _Refused("the stream has no IDAT")
    if hdr["color_type"] == 3 and palette is None:
        raise _Refused("colour type 3 without PLTE: a missing PLTE")
    hdr["palette"] = palette if hdr["color_type"] == 3 else None
    hdr["idat"] = idat  # the chunk bodies in order: inflate takes them one after the other, nothing is concatenated
    return hdr


def png_info(data, verify=True):
    """Header of one stream: {'height', 'width', 'color_type', 'depth', 'samples', 'rowbytes', 'bpp', 'palette_entries', 'idat_bytes'}.
    The whole chunk walk runs (every length bounds-checked, every CRC-32 verified unless verify=False); nothing is inflated.  A stream
    outside the accepted subset raises HpeError with the clause.  Pure host."""
    try:
        h = _parse(stream_list([data])[0][0], verify)
    except _Refused as e:
        raise _named(0, e) from None
    return {"height": h["H"], "width": h["W"], "color_type": h["color_type"], "depth": h["depth"], "samples": h["samples"],
            "rowbytes": h["rowbytes"], "bpp": h["bpp"], "palette_entries": len(h["palette"]) // 3 if h["palette"] else 0,
            "idat_bytes": sum(len(b) for b in h["idat"])}


def _run(pool, fn, items, indices):
    """fn over the items on the pool; the refusal of the lowest image is the one raised, whatever the thread count"""
    def guarded(x):
        try:
            return fn(x)
        except _Refused as e:
            return e

    results = list(pool.map(guarded, items)) if pool is not None else [guarded(x) for x in items]
    for i, r in zip(indices, results):
        if isinstance(r, _Refused):
            raise _named(i, r) from None
    return results


def parse_batch(streams, threads=DEFAULT_THREADS, verify=True, indices=None, pool=None):
    """The chunk walk of every stream -> a list of header dicts (``_parse``).  indices: the image numbers a refusal names (default 0..B-1)."""
    data, _ = stream_list(streams)
    indices = range(len(data)) if indices is None else indices
    if pool is not None or thread_count(threads) == 1:
        return _run(pool, lambda d: _parse(d, verify), data, indices)
    with ThreadPoolExecutor(max_workers=threads) as own:
        return _run(own, lambda d: _parse(d, verify), data, indices)


def _inflate(job):
    h, region = job
    H, rb = h["H"], h["rowbytes"]
    want = H * (rb + 1)
    d = zlib.decompressobj()
    pos = 0
    try:
        for part in h["idat"]:
            while len(part) and not d.eof and pos <= want:
                # capped at what is still missing plus one byte: a crafted stream cannot allocate more than its header promises
                out = d.decompress(part, want + 1 - pos)
                if pos + len(out) <= want:
                    region[pos:pos + len(out)] = np.frombuffer(out, np.uint8)
                pos += len(out)
                part = d.unconsumed_tail  # not empty only when the cap was reached
    except zlib.error as e:
        raise _Refused("the zlib stream errors: %s" % e) from None
    if pos != want:
        raise _Refused("the inflated data is %s %d bytes, not H * (1 + rowbytes) = %d" % ("more than" if pos > want else "only", min(pos, want), want))
    if not d.eof:
        raise _Refused("the zlib stream errors: it ends before its end marker")
    filters = region.reshape(H, rb + 1)[:, 0]  # one strided read of byte 0 of every row
    if int(filters.max()) > 4:
        y = int(np.argmax(filters > 4))
        raise _Refused("row %d has filter type %d, above 4" % (y, int(filters[y])))
    return None


def inflate_batch(streams, channels=3, threads=DEFAULT_THREADS, alloc=None, verify=True, out_offsets=None, indices=None, headers=None):
    """The host half alone: -> (staged uint8 [totals[0] + 64 * B], table record array [B] of ``TABLE_DTYPE`` -- a view of the staged buffer's
    tail --, totals int64 [4] = raw bytes (scanlines, then palettes), workspace bytes, frame bytes, workgroups of launch two).  Every
    image inflates into its own region of the ONE staged buffer, on a 16-byte boundary; the palettes follow, padded to 256 entries with
    zeros; the table comes last.  ``alloc(nbytes)`` may return the uint8 array to fill, e.g. a view of pinned memory.  out_offsets:
    frame offsets to use instead of the packing in order.  Any refused stream raises HpeError naming the image (the lowest one), before
    anything is inflated when its chunks are the reason.  The bytes do not depend on ``threads``.  Pure host code: no device is needed."""
    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    threads = thread_count(threads)
    data, _ = stream_list(streams)
    B = len(data)
    indices = list(range(B)) if indices is None else list(indices)
    pool = ThreadPoolExecutor(max_workers=threads) if threads > 1 else None
    try:
        hs = headers if headers is not None else parse_batch(data, threads, verify, indices, pool)
        table = np.zeros(B, TABLE_DTYPE)
        packed, frames_total = frame_offsets([(h["H"], h["W"]) for h in hs], channels)
        if out_offsets is not None:
            packed = np.ascontiguousarray(out_offsets, dtype=np.int64)
            if packed.shape != (B,):
                raise ValueError("out_offsets must hold one offset per stream")
        raw_pos = work_pos = groups = 0
        for b, h in enumerate(hs):
            e = table[b]
            for k in ("H", "W", "color_type", "depth", "rowbytes", "bpp"):
                e[k] = h[k]
            e["channels"], e["out_offset"], e["raw_offset"], e["store_group0"] = channels, packed[b], raw_pos, groups
            raw_pos += up16(h["H"] * (h["rowbytes"] + 1))
            if is_direct(h["color_type"], h["depth"], channels):
                e["work_offset"] = -1
            else:
                e["work_offset"] = work_pos
                work_pos += up16(h["H"] * h["rowbytes"])
                groups += (h["H"] * h["W"] * channels + STORE_BYTES_PER_GROUP - 1) // STORE_BYTES_PER_GROUP
        for b, h in enumerate(hs):
            table[b]["pal_offset"] = -1
            if h["color_type"] == 3:
                table[b]["pal_offset"] = raw_pos
                raw_pos += PALETTE_BYTES
        nbytes = raw_pos + B * TABLE_DTYPE.itemsize
        staged = alloc(nbytes) if alloc is not None else np.zeros(nbytes, np.uint8)
        if not isinstance(staged, np.ndarray) or staged.dtype != np.uint8 or staged.shape != (nbytes,) or not staged.flags.c_contiguous:
            raise ValueError("alloc must return a contiguous uint8 [nbytes] array")
        jobs = []
        for b, h in enumerate(hs):
            o, n = int(table[b]["raw_offset"]), h["H"] * (h["rowbytes"] + 1)
            staged[o + n:o + up16(n)] = 0  # the bytes between the regions are defined too
            jobs.append((h, staged[o:o + n]))
            if h["color_type"] == 3:
                pal = staged[int(table[b]["pal_offset"]):int(table[b]["pal_offset"]) + PALETTE_BYTES].reshape(256, 4)
                pal[:] = 0
                pal[:len(h["palette"]) // 3, :3] = np.frombuffer(h["palette"], np.uint8).reshape(-1, 3)
        _run(pool, _inflate, jobs, indices)
    finally:
        if pool is not None:
            pool.shutdown()
    staged[raw_pos:].view(TABLE_DTYPE)[:] = table
    return staged, staged[raw_pos:].view(TABLE_DTYPE), np.array([raw_pos, max(work_pos, 16), frames_total, groups], np.int64)


def _pinned_alloc(keep):
    def alloc(nbytes):
        buf, host = pinned(nbytes)
        keep.append(buf)
        return host

    return alloc


def _launch_png(pinned_buf, table, totals, out, dev):
    """one non-blocking copy of the staged buffer and the two launches on the current stream"""
    import torch

    raw_bytes = int(totals[0])
    staged = upload(pinned_buf, dev)
    workspace = torch.empty(int(totals[1]), dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().hpe_png_backend(_p(table), staged.data_ptr() + raw_bytes, table.shape[0], staged.data_ptr(), raw_bytes,
                                           workspace.data_ptr(), workspace.numel(), out.data_ptr(), out.numel(), stream_ptr(dev)))


def decode_png_batch(streams, channels=3, threads=DEFAULT_THREADS, out=None):
    """Every PNG stream decoded as ``tf.image.decode_jpeg(s, channels=channels)`` decodes it -> ``DecodedBatch`` on the current CUDA
    device.  channels is 1 or 3 for the whole batch: grey replicates to 3, colour goes to 1 by libpng's rgb_to_gray weights, a palette
    is looked up, alpha is dropped.  The inflated scanlines, the palettes and the table are written into ONE pinned buffer, go up in one
    non-blocking copy, and the two launches follow on the current stream; nothing reads the device.  A refused stream raises HpeError
    naming its index before anything is launched.  out: an optional contiguous uint8 CUDA tensor to decode into (at least the packed
    size; bytes between and after the frames are left as they are)."""
    import torch

    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    dev = check_out(out)
    keep = []
    with torch.cuda.device(dev):
        _, table, totals = inflate_batch(streams, channels, threads, _pinned_alloc(keep))
        out = frames_out(out, int(totals[2]), dev)
        _launch_png(keep[0], table, totals, out, dev)
    sizes = np.stack([table["H"], table["W"]], axis=1).astype(np.int64)
    return DecodedBatch(out, sizes, table["out_offset"].astype(np.int64), channels)


def sniff(data):
    """'jpeg', 'png' or None by the stream's first bytes"""
    head = bytes(data[:8])
    return "png" if head == SIGNATURE else "jpeg" if head[:2] == JPEG_SOI else None


def decode_image_batch(streams, channels, threads=DEFAULT_THREADS, out=None):
    """``decode_jpeg_batch`` and ``decode_png_batch`` in one: every stream is taken by its signature (JPEG's SOI or PNG's eight bytes; a
    stream that is neither is refused with its index), ONE packed buffer is laid out in batch order, and the JPEG subset and the PNG
    subset both decode straight into it -- the offsets of both tables are written here, there is no gather copy.  All host work (entropy
    decode, chunk walk, inflate) comes first: a refused stream raises HpeError naming its index in ``streams`` before anything is
    launched.  Same arguments and result as the two."""
    import torch

    from . import jpeg

    if channels not in (1, 3):
        raise ValueError("channels must be 1 or 3")
    data, _ = stream_list(streams)
    threads = thread_count(threads)
    dev = check_out(out)
    kinds = [sniff(s) for s in data]
    for i, k in enumerate(kinds):
        if k is None:
            raise HpeError("image %d: neither a JPEG nor a PNG stream (no SOI, no PNG signature)" % i)
    ji = [i for i, k in enumerate(kinds) if k == "jpeg"]
    pi = [i for i, k in enumerate(kinds) if k == "png"]
    B = len(data)
    sizes = np.zeros((B, 2), np.int64)
    pinned_j, pinned_p = [], []

    with torch.cuda.device(dev):
        headers = parse_batch([data[i] for i in pi], threads, True, pi) if pi else []
        if ji:
            try:
                _, jtable, jtotals = jpeg.entropy_decode([data[i] for i in ji], channels, threads, jpeg._pinned_alloc(pinned_j))
            except HpeError as e:  # the subset's numbering -> the batch's
                raise HpeError(re.sub(r"image (\d+)", lambda m: "image %d" % ji[int(m.group(1))], str(e), count=1)) from None
            sizes[ji] = np.stack([jtable["H"], jtable["W"]], axis=1)
        if pi:
            sizes[pi] = [(h["H"], h["W"]) for h in headers]
        offsets, need = frame_offsets(sizes, channels)
        if pi:
            _, ptable, ptotals = inflate_batch([data[i] for i in pi], channels, threads, _pinned_alloc(pinned_p), out_offsets=offsets[pi],
                                               indices=pi, headers=headers)
        out = frames_out(out, need, dev)
        if ji:
            jtable["out_offset"] = offsets[ji]  # hpe_jpeg_backend takes any 16-byte aligned offset inside the buffer
            jpeg._launch_jpeg(pinned_j[0], jtable, jtotals, out, dev)
        if pi:
            _launch_png(pinned_p[0], ptable, ptotals, out, dev)
    return DecodedBatch(out, sizes, offsets, channels)
