"""The host half of the JPEG decoder without a GPU: the library's entropy decode (hpe_jpeg_decode) fed through the NumPy restatement of
the back end (tests/jpeg_ref.py) equals, bit for bit, the pixels libjpeg-turbo decoded when the fixtures were made
(tests/golden/make_jpeg_golden.py); the bytes do not depend on the thread count; everything outside the accepted subset, every
truncation and every damaged stream is refused or decoded without a write outside the buffers it was given."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_ref as R
from hpe_amd import HpeError, _lib, batch_io, build as hbuild, jpeg


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


@pytest.fixture(scope="module")
def decoded(lib):
    """every fixture decoded once per channel count, as one mixed batch: name -> (coef, table entry)"""
    out = {}
    for ch in (3, 1):
        coef, table, _ = jpeg.entropy_decode([R.stream(n) for n in R.CASES], ch, threads=2)
        coef.setflags(write=False)
        for n, e in zip(R.CASES, table):
            out[n, ch] = (coef, e)
    return out


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("name", R.CASES)
def test_entropy_decode_through_restatement_equals_golden(decoded, name, channels):
    coef, entry = decoded[name, channels]
    got = R.decode(coef, entry)
    want = R.golden(name, channels)
    if channels == 1:
        got = got[:, :, 0]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


def test_clamp_case_reaches_both_ends():
    g = R.golden("noise_q100_48x48", 3)
    assert g.min() == 0 and g.max() == 255


@pytest.mark.parametrize("name", R.CASES)
def test_goldens_equal_pillow_today(name):
    Image = pytest.importorskip("PIL.Image")
    data = R.stream(name)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), R.golden(name, 3))
    im = Image.open(io.BytesIO(data))
    im.draft("L", im.size)
    assert np.array_equal(np.asarray(im), R.golden(name, 1))


def test_info(lib):
    i = jpeg.jpeg_info(R.stream("s420_37x43"))
    assert i == {"height": 37, "width": 43, "components": 3, "sampling": [(2, 2), (1, 1), (1, 1)], "blocks": [(6, 6), (3, 3), (3, 3)],
                 "coefficients": 64 * (36 + 9 + 9)}
    i = jpeg.jpeg_info(R.stream("s422_17x35"))
    assert i["sampling"][0] == (2, 1) and i["blocks"] == [(3, 6), (3, 3), (3, 3)]
    i = jpeg.jpeg_info(R.stream("grey_23x9"))
    assert i["components"] == 1 and i["blocks"] == [(3, 2)] and i["coefficients"] == 64 * 6


def test_one_channel_of_a_colour_stream_stores_luma_only(decoded):
    _, e3 = decoded["s420_37x43", 3]
    _, e1 = decoded["s420_37x43", 1]
    assert (e3["ncomp"], e3["hmax"], e3["vmax"]) == (3, 2, 2) and (e1["ncomp"], e1["hmax"], e1["vmax"], e1["channels"]) == (1, 2, 2, 1)
    assert e1["blocks_w"].tolist() == [6, 0, 0] and np.array_equal(e1["quant"][0], e3["quant"][0]) and not e1["quant"][1:].any()


def test_thread_count_does_not_change_the_bytes(lib):
    streams = [R.stream(n) for n in R.CASES] * 2
    ch = [3, 1] * len(R.CASES)
    c1, t1, tot1 = jpeg.entropy_decode(streams, ch, threads=1)
    c4, t4, tot4 = jpeg.entropy_decode(streams, ch, threads=4)
    assert c1.tobytes() == c4.tobytes() and t1.tobytes() == t4.tobytes() and tot1.tolist() == tot4.tolist()


def test_layout_packs_on_boundaries(lib):
    streams = [R.stream(n) for n in R.CASES]
    _, table, totals = jpeg.entropy_decode(streams, 3, threads=1)
    off = 0
    for e in table:
        assert e["out_offset"] == off and off % 16 == 0
        off += (int(e["H"]) * int(e["W"]) * 3 + 15) // 16 * 16
    assert totals[2] == off and totals[0] == totals[1] and (table["coef_offset"] % 8 == 0).all()
    assert (np.diff(table["idct_group0"]) >= 1).all() and (np.diff(table["store_group0"]) >= 1).all()


def _refused(streams, channels=3, threads=1, match=None):
    with pytest.raises(HpeError, match=match):
        jpeg.entropy_decode(streams, channels, threads)


def test_progressive_is_refused(lib):
    _refused([R.stream(R.REFUSED[0])], match="image 0: progressive")
    with pytest.raises(HpeError, match="progressive"):
        jpeg.jpeg_info(R.stream(R.REFUSED[0]))


def test_a_refused_stream_in_a_batch_is_named(lib):
    ok = R.stream("s444_19x21")
    _refused([ok, R.stream(R.REFUSED[0]), ok], match="image 1: progressive")
    _refused([ok, ok, ok[:-2]], threads=3, match="image 2: ")


def test_not_a_jpeg_is_refused(lib):
    _refused([b"\x89PNG\r\n\x1a\n" + bytes(64)], match="no SOI")
    _refused([R.stream("s444_19x21")[2:]], match="no SOI")
    _refused([b""], match="no SOI")


def test_bad_arguments_are_refused(lib):
    ok = [R.stream("s444_19x21")]
    for ch in (0, 2, 4):
        _refused(ok, channels=ch, match="channels must be 1 or 3")
    for th in (0, 17, -1):
        _refused(ok, threads=th, match=r"threads must be in \[1, 16\]")


def _smallest_colour():
    return min((R.stream(n) for n in R.CASES if not n.startswith("grey")), key=len)


def test_every_prefix_is_refused(lib):
    s = _smallest_colour()
    for n in range(len(s)):
        with pytest.raises(HpeError):
            jpeg.entropy_decode([s[:n]], 3, threads=1)
    jpeg.entropy_decode([s], 3, threads=1)


def test_single_byte_damage_returns_a_status_and_stays_inside_the_buffer(lib):
    """every byte of the first 700 set to 0x00 and to 0xFF: success or an error status, and the canaries around the coefficient buffer
    and the table stay intact"""
    s = _smallest_colour()
    guard = 256
    seen = {"ok": 0, "refused": 0}
    store = {}

    def alloc(n, B):
        store["coef"] = np.full(n + 2 * guard, 0x5A5A, np.int16)
        store["table"] = np.zeros(B + 2, jpeg.TABLE_DTYPE)
        store["table"].view(np.uint8)[:] = 0xC3
        return store["coef"][guard:guard + n], store["table"][1:1 + B]

    for pos in range(min(700, len(s))):
        for v in (0x00, 0xFF):
            m = bytearray(s)
            m[pos] = v
            store.clear()
            try:
                jpeg.entropy_decode([bytes(m)], 3, threads=1, alloc=alloc)
                seen["ok"] += 1
            except HpeError:
                seen["refused"] += 1
            if store:
                c, t = store["coef"], store["table"].view(np.uint8).reshape(-1, jpeg.TABLE_DTYPE.itemsize)
                assert (c[:guard] == 0x5A5A).all() and (c[-guard:] == 0x5A5A).all() and (t[0] == 0xC3).all() and (t[-1] == 0xC3).all(), (pos, v)
    assert seen["ok"] > 0 and seen["refused"] > 0, seen


def test_capacity_is_checked_before_anything_is_written(lib):
    s = R.stream("s420_37x43")
    data, lengths = batch_io.stream_list([s])
    ptrs = (C.c_char_p * 1)(*data)
    ch = np.array([3], np.int32)
    status, totals, table = np.zeros(1, np.int32), np.zeros(5, np.int64), np.zeros(1, jpeg.TABLE_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.hpe_jpeg_decode(1, ptrs, p(lengths), p(ch), 1, None, 0, p(table), p(status), p(totals)) == 0
    n = int(totals[0])
    coef = np.full(n, 0x5A5A, np.int16)
    assert lib.hpe_jpeg_decode(1, ptrs, p(lengths), p(ch), 1, p(coef), n - 1, p(table), p(status), p(totals)) == 1
    assert b"coef_capacity" in lib.hpe_last_error() and (coef == 0x5A5A).all()
    assert lib.hpe_jpeg_decode(1, ptrs, p(lengths), p(ch), 1, p(coef), n, p(table), p(status), p(totals)) == 0 and status[0] == 0


def test_backend_checks_the_table_before_any_launch(lib):
    """hpe_jpeg_backend refuses an entry that points outside the buffers it was given; the check comes before the first HIP call, so it
    runs without a GPU (the pointers are never dereferenced)"""
    _, table, totals = jpeg.entropy_decode([R.stream("s420_37x43"), R.stream("s422_17x35")], 3, threads=1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    fake = 1 << 20  # aligned, never dereferenced: every call below is refused

    def call(t, coefs=int(totals[0]), ws=int(totals[1]), fr=int(totals[2])):
        return lib.hpe_jpeg_backend(p(t), fake, 2, fake, coefs, fake, ws, fake, fr, None)

    for field, value, clause in (("out_offset", int(totals[2]), b"frame"), ("out_offset", 8, b"frame"), ("coef_offset", [0, 0, int(totals[0])], b"coefficients"),
                                 ("plane_offset", [0, 0, -64], b"plane"), ("H", 0, b"H and W"), ("blocks_w", [7, 3, 3], b"block grid"),
                                 ("store_group0", 0, b"workgroup"), ("hmax", 3, b"sampling"), ("channels", 1, b"channels")):
        bad = table.copy()
        bad[field][1] = value
        assert call(bad) == 1 and b"table entry 1" in lib.hpe_last_error() and clause in lib.hpe_last_error(), (field, lib.hpe_last_error())
    last = int(table["out_offset"][1]) + int(table["H"][1]) * int(table["W"][1]) * 3  # the end of the last frame; totals[2] rounds it up to 16
    assert call(table, coefs=int(totals[0]) - 1) == 1 and call(table, ws=int(totals[1]) - 1) == 1 and call(table, fr=last - 1) == 1
