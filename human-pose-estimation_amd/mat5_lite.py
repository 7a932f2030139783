"""A minimal reader of MATLAB level-5 ``.mat`` files, for the label files of the dataset writers (``joints.mat`` of LSP and LSP-extended,
src/util/create_dataset.py:11-15) without scipy: ``load(path)`` -> {name: array} of the file's real numeric matrices.  Little-endian
files, miMATRIX elements of the numeric classes (double, single, the 8- to 64-bit integers; a logical array comes back as bool), also
inside miCOMPRESSED elements (zlib).  Everything else -- cell, struct, object, char and sparse arrays, complex data, big-endian files,
level-4 and HDF5-based (v7.3) files -- is refused by name; nothing is read "as far as it goes".  Pure host code."""
from __future__ import annotations

import struct
import zlib

import numpy as np

MI_TYPES = {1: "i1", 2: "u1", 3: "<i2", 4: "<u2", 5: "<i4", 6: "<u4", 7: "<f4", 9: "<f8", 12: "<i8", 13: "<u8"}
MI_MATRIX, MI_COMPRESSED = 14, 15
MX_CLASSES = {6: np.float64, 7: np.float32, 8: np.int8, 9: np.uint8, 10: np.int16, 11: np.uint16, 12: np.int32, 13: np.uint32, 14: np.int64,
              15: np.uint64}
MX_REFUSED = {1: "a cell array", 2: "a struct array", 3: "an object", 4: "a char array", 5: "a sparse array", 16: "a function handle",
              17: "an opaque object"}
MAX_INFLATED = 1 << 31


class MatError(ValueError):
    pass


def _element(buf, pos, what):
    """the data element at ``pos`` -> (type, payload memoryview, position of the next element)"""
    if len(buf) - pos < 8:
        raise MatError("%s: truncated: a tag of 8 bytes at offset %d runs past the end" % (what, pos))
    first, nbytes = struct.unpack_from("<II", buf, pos)
    if first >> 16:  # the small element format: the size in the upper half, the data in the tag itself
        nbytes, kind = first >> 16, first & 0xFFFF
        if nbytes > 4:
            raise MatError("%s: a small data element of %d bytes" % (what, nbytes))
        return kind, memoryview(buf)[pos + 4:pos + 4 + nbytes], pos + 8
    start = pos + 8
    if nbytes > len(buf) - start:
        raise MatError("%s: truncated: an element of %d bytes at offset %d runs past the end" % (what, nbytes, pos))
    end = start + nbytes
    return first, memoryview(buf)[start:end], end if first == MI_COMPRESSED else (end + 7) // 8 * 8


def _numbers(kind, payload, what):
    if kind not in MI_TYPES:
        raise MatError("%s: data type %d is not a numeric type" % (what, kind))
    dt = np.dtype(MI_TYPES[kind])
    if len(payload) % dt.itemsize:
        raise MatError("%s: %d bytes of a %d-byte type" % (what, len(payload), dt.itemsize))
    return np.frombuffer(payload, dt)


def _matrix(body, what):
    """the subelements of one miMATRIX -> (name, array)"""
    body = bytes(body)
    kind, flags, pos = _element(body, 0, what)
    if kind != 6 or len(flags) != 8:
        raise MatError("%s: a matrix without array flags" % what)
    word = struct.unpack_from("<I", flags, 0)[0]
    mx, is_complex, is_logical = word & 0xFF, bool(word & 0x0800), bool(word & 0x0200)
    kind, dims, pos = _element(body, pos, what)
    dims = _numbers(kind, dims, what).astype(np.int64)
    kind, name, pos = _element(body, pos, what)
    name = bytes(name).decode("latin-1")
    label = "%s: variable '%s'" % (what, name)
    if mx in MX_REFUSED:
        raise MatError("%s is %s: only real numeric matrices are read" % (label, MX_REFUSED[mx]))
    if mx not in MX_CLASSES:
        raise MatError("%s has the unknown class %d" % (label, mx))
    if is_complex:
        raise MatError("%s is complex: only real numeric matrices are read" % label)
    if kind != 1 or len(dims) < 2 or (dims < 0).any():
        raise MatError("%s: a malformed name or dimensions" % label)
    kind, data, pos = _element(body, pos, label)
    values = _numbers(kind, data, label)
    count = int(np.prod(dims))
    if values.size != count:
        raise MatError("%s: %d values for dimensions %s" % (label, values.size, dims.tolist()))
    out = values.astype(MX_CLASSES[mx]).reshape(tuple(int(d) for d in dims), order="F")
    return name, (out.astype(bool) if is_logical else np.ascontiguousarray(out))


def load(path):
    """-> {name: array} of every variable of the file, in file order"""
    with open(path, "rb") as f:
        buf = f.read()
    what = str(path)
    if buf[:8] == b"\x89HDF\r\n\x1a\n" or buf[:10] == b"MATLAB 7.3":
        raise MatError("%s: an HDF5-based (v7.3) file: only level-5 files are read" % what)
    if len(buf) < 128:
        raise MatError("%s: truncated: %d bytes, the header alone has 128" % (what, len(buf)))
    if buf[126:128] == b"MI":
        raise MatError("%s: a big-endian file: only little-endian files are read" % what)
    if buf[126:128] != b"IM" or not buf[:4].strip(b"\0") or struct.unpack_from("<H", buf, 124)[0] != 0x0100:
        raise MatError("%s: not a level-5 MAT-file (level-4 files are not read)" % what)
    out, pos = {}, 128
    while pos < len(buf):
        kind, payload, pos = _element(buf, pos, what)
        if kind == MI_COMPRESSED:
            try:
                d = zlib.decompressobj()
                inner = d.decompress(bytes(payload), MAX_INFLATED)
                if not d.eof:
                    raise MatError("%s: truncated: a compressed element ends early" % what)
            except zlib.error as e:
                raise MatError("%s: a compressed element does not inflate: %s" % (what, e)) from e
            kind, payload, _ = _element(inner, 0, what)
        if kind != MI_MATRIX:
            raise MatError("%s: a top-level element of type %d, not a matrix" % (what, kind))
        name, arr = _matrix(payload, what)
        out[name] = arr
    if not out:
        raise MatError("%s: the file holds no variable" % what)
    return out
