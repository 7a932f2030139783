"""batch_io and the record dtypes derived from the ctypes structures of _lib.py: pure host, no library call.  The field lists below are
the hand-written dtypes these records had before they were derived; a reordered, renamed or resized field fails here."""
import ctypes as C

import numpy as np
import pytest

from hpe_amd import HpeError, _lib, augment, batch_io, jpeg, jpeg_encode, png, png_encode

RECORDS = {
    "jpeg.INFO_DTYPE": (jpeg.INFO_DTYPE, _lib.HpeJpegInfo, 72, [
        ("status", "<i4"), ("H", "<i4"), ("W", "<i4"), ("ncomp", "<i4"), ("hs", "<i4", 3), ("vs", "<i4", 3), ("blocks_w", "<i4", 3),
        ("blocks_h", "<i4", 3), ("coefs", "<i8")]),
    "jpeg.TABLE_DTYPE": (jpeg.TABLE_DTYPE, _lib.HpeJpegImage, 304, [
        ("coef_offset", "<i8", 3), ("plane_offset", "<i8", 3), ("out_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("ncomp", "<i4"),
        ("channels", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"), ("blocks_w", "<i4", 3), ("blocks_h", "<i4", 3), ("idct_group0", "<i4"),
        ("store_group0", "<i4"), ("quant", "u1", (3, 64))]),
    "jpeg_encode.ENC_DTYPE": (jpeg_encode.ENC_DTYPE, _lib.HpeJpegEncImage, 232, [
        ("frame_offset", "<i8"), ("coef_offset", "<i8", 3), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("hmax", "<i4"), ("vmax", "<i4"),
        ("blocks_w", "<i4", 3), ("blocks_h", "<i4", 3), ("real_w", "<i4", 3), ("real_h", "<i4", 3), ("group0", "<i4"),
        ("quant", "u1", (2, 64))]),
    "png.TABLE_DTYPE": (png.TABLE_DTYPE, _lib.HpePngImage, 64, [
        ("raw_offset", "<i8"), ("pal_offset", "<i8"), ("work_offset", "<i8"), ("out_offset", "<i8"), ("H", "<i4"), ("W", "<i4"),
        ("color_type", "<i4"), ("depth", "<i4"), ("channels", "<i4"), ("rowbytes", "<i4"), ("bpp", "<i4"), ("store_group0", "<i4")]),
    "png_encode.FILTER_DTYPE": (png_encode.FILTER_DTYPE, _lib.HpePngFilterImage, 32, [
        ("frame_offset", "<i8"), ("scan_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("row0", "<i4")]),
    "augment.TABLE_DTYPE": (augment.TABLE_DTYPE, _lib.HpeAugmentFrame, 64, [
        ("frame_offset", "<i8"), ("seg_offset", "<i8"), ("H", "<i4"), ("W", "<i4"), ("newH", "<i4"), ("newW", "<i4"), ("cx", "<i4"),
        ("cy", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("flip", "<i4"), ("inside", "<i4"), ("rx", "<f4"), ("ry", "<f4")]),
}


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_record_dtype_is_the_hand_written_layout(name):
    derived, struct, itemsize, fields = RECORDS[name]
    want = np.dtype(fields)  # packed, in the order written: the offsets are the running sum
    assert derived.names == want.names == tuple(f[0] for f in fields)
    for f in want.names:
        (dt, off), (wdt, woff) = derived.fields[f][:2], want.fields[f][:2]
        assert (off, dt.shape, dt.base) == (woff, wdt.shape, wdt.base), f
    assert derived.itemsize == want.itemsize == itemsize == C.sizeof(struct)


def test_up16_and_frame_offsets():
    assert [batch_io.up16(n) for n in (0, 1, 15, 16, 17, 32)] == [0, 16, 16, 16, 32, 32]
    sizes = [(4, 4), (1, 17), (1, 1), (3, 5)]  # 16 bytes exactly, 17, 1, 15
    offs, total = batch_io.frame_offsets(sizes, 1)
    assert offs.dtype == np.int64 and offs.tolist() == [0, 16, 48, 64] and total == 80
    offs3, total3 = batch_io.frame_offsets(sizes, 3)  # 48, 51, 3, 45
    assert offs3.tolist() == [0, 48, 112, 128] and total3 == 176
    assert batch_io.DecodedBatch(None, np.array(sizes, np.int64), offs, 1).nbytes == total
    assert batch_io.DecodedBatch(None, np.array(sizes, np.int64), offs3, 3).nbytes == total3
    assert batch_io.DecodedBatch(None, np.array(sizes[:1], np.int64), offs[:1], 1).nbytes == 16  # no padding piece
    assert batch_io.DecodedBatch(None, np.array(sizes[:3], np.int64), offs[:3], 1).nbytes == 64
    assert jpeg.DecodedBatch is batch_io.DecodedBatch and png.frame_offsets is batch_io.frame_offsets


def test_stream_list():
    for bad, clause in ((b"abc", "streams must be a list of bytes objects"), (7, "streams must be a list of bytes objects"),
                        ([], "streams is empty"), ([b"ab", "cd"], "every stream must be bytes-like"), ([None], "every stream must be bytes-like")):
        with pytest.raises(ValueError) as e:
            batch_io.stream_list(bad)
        assert str(e.value) == clause
    data, lengths = batch_io.stream_list([b"ab", bytearray(b"cde"), memoryview(b"f"), np.frombuffer(b"ghij", np.uint8), b""])
    assert data == [b"ab", b"cde", b"f", b"ghij", b"\0"] and all(type(d) is bytes for d in data)
    assert lengths.dtype == np.int64 and lengths.tolist() == [2, 3, 1, 4, 0]  # the stand-in has an address, the length stays 0


@pytest.mark.parametrize("error, clause", [(ValueError, "threads must be an integer in [1, 16]"),
                                           (HpeError, "threads must be an integer in [1, 16], got %r")])
def test_thread_count(error, clause):
    for bad in (0, 17, 2.5):
        with pytest.raises(error) as e:
            batch_io.thread_count(bad, error)
        assert str(e.value) == (clause % (bad,) if "%" in clause else clause)
    assert batch_io.thread_count(16, error) == 16 and batch_io.thread_count(1, error) == 1
    assert type(batch_io.thread_count(4.0, error)) is int


def test_the_codecs_refuse_as_before():
    with pytest.raises(ValueError, match=r"^threads must be an integer in \[1, 16\]$"):
        png.parse_batch([b"x"], threads=0)
    with pytest.raises(ValueError, match=r"^threads must be an integer in \[1, 16\]$"):
        png_encode.deflate_batch(np.zeros(2, np.uint8), np.zeros(1, png_encode.FILTER_DTYPE), threads=17)
    with pytest.raises(HpeError, match=r"^threads must be an integer in \[1, 16\], got 2\.5$"):
        jpeg_encode.entropy_encode(np.zeros(64, np.int16), np.zeros(1, jpeg_encode.ENC_DTYPE), threads=2.5)
