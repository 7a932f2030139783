"""Writer of PNG streams for the tests: the inverse of hpe_amd.png, written from the format's definition (PNG 1.2 sections 3, 4, 6, 9) and
sharing nothing with the reader.  It does the forward filtering itself, with the filter type forced per row, and compresses with
``zlib.compress``; any accepted colour type and depth, an optional PLTE, IDAT cut into chunks of any size, extra chunks anywhere."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind, body=b"", crc=None):
    crc = zlib.crc32(kind + body) if crc is None else crc
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", crc & 0xFFFFFFFF)


def ihdr(W, H, depth, color_type, compression=0, filter_method=0, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, color_type, compression, filter_method, interlace))


def pack_rows(samples, depth):
    """samples uint8 [H, W, spp] (values below 2^depth) -> the unfiltered rows uint8 [H, rowbytes]: leftmost pixel in the high bits"""
    H, W, spp = samples.shape
    if depth == 8:
        return np.ascontiguousarray(samples.reshape(H, W * spp))
    assert spp == 1 and int(samples.max(initial=0)) < (1 << depth)
    per = 8 // depth
    padded = np.zeros((H, -(-W // per) * per), np.uint8)
    padded[:, :W] = samples[:, :, 0]
    out = np.zeros((H, padded.shape[1] // per), np.uint8)
    for k in range(per):
        out |= padded[:, k::per] << (8 - depth * (k + 1))
    return out


def filter_rows(rows, bpp, filters):
    """rows uint8 [H, rowbytes], filters: one type for all rows or one per row -> the scanlines uint8 [H, 1 + rowbytes]"""
    H, rb = rows.shape
    filters = [filters] * H if np.isscalar(filters) else list(filters)
    assert len(filters) == H
    cur = np.zeros((H + 1, rb + bpp), np.int64)  # a row of zeros above, bpp zeros to the left
    cur[1:, bpp:] = rows
    out = np.zeros((H, rb + 1), np.uint8)
    for y, ft in enumerate(filters):
        x = cur[y + 1, bpp:]
        a, b, c = cur[y + 1, :rb], cur[y, bpp:], cur[y, :rb]
        if ft == 0:
            pred = np.zeros(rb, np.int64)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = b
        elif ft == 3:
            pred = (a + b) // 2
        elif ft == 4:
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)  # |p - a|, |p - b|, |p - c| with p = a + b - c
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        else:  # an invalid type, for the refusal tests: stored as it is, the bytes unfiltered
            pred = np.zeros(rb, np.int64)
        out[y, 0] = ft
        out[y, 1:] = (x - pred) % 256
    return out


def write_png(samples, color_type, depth=8, filters=0, palette=None, idat_size=None, before_idat=(), after_idat=(), level=6, interlace=0,
              scanlines=None, end=True):
    """samples uint8 [H, W, spp] of raw sample values (palette indices for colour type 3) -> the stream.  palette: uint8 [n, 3].
    idat_size: cut the compressed data into IDAT chunks of that many bytes.  before_idat / after_idat: (kind, body) chunks placed after
    PLTE and after the last IDAT.  scanlines: bytes to compress instead of the filtered rows (for the refusal tests)."""
    samples = np.asarray(samples, np.uint8)
    H, W, spp = samples.shape
    assert spp == SAMPLES[color_type]
    bpp = max(1, spp * depth // 8)
    raw = filter_rows(pack_rows(samples, depth), bpp, filters).tobytes() if scanlines is None else scanlines
    data = zlib.compress(raw, level)
    out = [SIGNATURE, ihdr(W, H, depth, color_type, interlace=interlace)]
    if palette is not None:
        out.append(chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes()))
    out += [chunk(k, b) for k, b in before_idat]
    step = len(data) if not idat_size else idat_size
    out += [chunk(b"IDAT", data[i:i + step]) for i in range(0, len(data), step)]
    out += [chunk(k, b) for k, b in after_idat]
    if end:
        out.append(chunk(b"IEND"))
    return b"".join(out)


def chunks_of(stream):
    """-> [(kind, body)] of a well-formed stream"""
    pos, out = 8, []
    while pos < len(stream):
        n, kind = struct.unpack(">I4s", stream[pos:pos + 8])
        out.append((kind, stream[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def from_chunks(chunks):
    return SIGNATURE + b"".join(chunk(k, b) for k, b in chunks)
