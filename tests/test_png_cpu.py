"""The host half of the PNG decoder without a GPU: the chunk walk and inflate (hpe_amd.png.inflate_batch) fed through the NumPy
restatement of the back end (tests/png_ref.py) equals, bit for bit, the arrays the fixtures were written from
(tests/golden/make_png_golden.py) and, where Pillow is importable, Pillow's decode; the bytes do not depend on the thread count;
everything outside the accepted subset, every truncation and every stream that inflates to another size than its header promises is
refused with its clause and its image index; and the table check of hpe_png_backend refuses damaged entries and short buffers before
anything could be launched (it is called with NULL device pointers)."""
import ctypes as C
import io
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

import png_ref as R
import png_writer as PW
from hpe_amd import HpeError, _lib, build as hbuild, png

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_png_golden as G  # noqa: E402

ALL = tuple(G.CASES)


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


@pytest.fixture(scope="module")
def streams():
    return [R.stream(n) for n in ALL]


@pytest.fixture(scope="module")
def decoded(streams):
    """{channels: (staged, table, totals, [png_ref.decode of every image])}: computed once"""
    out = {}
    for ch in (3, 1):
        staged, table, totals = png.inflate_batch(streams, ch, threads=2)
        out[ch] = (staged, table, totals, [R.decode(staged, e) for e in table])
    return out


@pytest.mark.parametrize("channels", [3, 1])
def test_host_parse_through_the_reference_equals_the_written_arrays(decoded, channels):
    for name, got in zip(ALL, decoded[channels][3]):
        want = G.truth(name, channels)
        assert got.shape == want.shape and got.dtype == np.uint8 and np.array_equal(got, want), (name, channels)


def test_the_committed_streams_are_what_the_generator_writes(streams):
    """the fixtures carry the filters, chunk cuts and extra chunks the generator asks for (zlib's bytes may differ between versions: the
    inflated scanlines are compared, not the files)"""
    for name, s in zip(ALL, streams):
        a, b = PW.chunks_of(s), PW.chunks_of(G.write(name))
        assert [k for k, _ in a if k != b"IDAT"] == [k for k, _ in b if k != b"IDAT"], name
        inflate = lambda cs: zlib.decompress(b"".join(body for k, body in cs if k == b"IDAT"))  # noqa: E731
        assert inflate(a) == inflate(b), name
    cuts = {n: [len(b) for k, b in PW.chunks_of(R.stream(n)) if k == b"IDAT"] for n in ("g8_5x5_idat1", "rgb_3x5_idat7")}
    assert set(cuts["g8_5x5_idat1"]) == {1} and len(cuts["g8_5x5_idat1"]) > 20 and set(cuts["rgb_3x5_idat7"][:-1]) == {7}
    H = G.CASES["g8_65x67_cycle"][0]
    raw = np.frombuffer(zlib.decompress(PW.chunks_of(R.stream("g8_65x67_cycle"))[1][1]), np.uint8).reshape(H, -1)
    assert raw[:10, 0].tolist() == [4, 3, 2, 1, 0, 4, 3, 2, 1, 0]


def test_pillow_agrees_where_it_is_importable(streams, decoded):
    """native channel count and grey to RGB; Pillow's convert("L") is another formula and is no yardstick for colour to grey"""
    Image = pytest.importorskip("PIL.Image")
    checked = 0
    for i, (name, s) in enumerate(zip(ALL, streams)):
        c = G.case(name)
        im = Image.open(io.BytesIO(s))
        ct = c["color_type"]
        if ct in (0, 4):
            grey = np.asarray(im)[:, :, 0] if im.mode == "LA" else np.asarray(im.convert("L"))
            assert np.array_equal(decoded[1][3][i], grey), name
            assert np.array_equal(decoded[3][3][i], np.repeat(grey[:, :, None], 3, axis=2)), name
            if im.mode in ("1", "L"):
                assert np.array_equal(decoded[3][3][i], np.asarray(im.convert("RGB"))), name
        elif ct in (2, 6):
            assert np.array_equal(decoded[3][3][i], np.asarray(im)[:, :, :3]), name
        elif int(c["samples"].max()) < len(c["palette"]):  # Pillow's own rule for an index beyond PLTE is not ours to test
            assert np.array_equal(decoded[3][3][i], np.asarray(im.convert("RGB"))), name
        else:
            continue
        checked += 1
    assert checked >= len(ALL) - 2


def test_png_info(streams):
    i = png.png_info(R.stream("p2_65x5_f4"))
    assert i == {"height": 65, "width": 5, "color_type": 3, "depth": 2, "samples": 1, "rowbytes": 2, "bpp": 1, "palette_entries": 4,
                 "idat_bytes": i["idat_bytes"]} and i["idat_bytes"] > 0
    i = png.png_info(R.stream("rgba_65x3_f3"))
    assert (i["height"], i["width"], i["color_type"], i["depth"], i["rowbytes"], i["bpp"]) == (65, 3, 6, 8, 12, 4)
    i = png.png_info(R.stream("g1_65x9_cycle"))
    assert (i["rowbytes"], i["bpp"], i["samples"]) == (2, 1, 1)


@pytest.mark.parametrize("channels", [3, 1])
def test_thread_count_does_not_change_the_bytes(streams, channels):
    a, ta, tota = png.inflate_batch(streams, channels, threads=1)
    b, tb, totb = png.inflate_batch(streams, channels, threads=4)
    assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes() and np.array_equal(tota, totb)
    for bad in (0, 17, 2.5):
        with pytest.raises(ValueError, match="threads"):
            png.inflate_batch(streams, channels, threads=bad)


def test_layout_of_the_staged_buffer(decoded):
    for ch in (3, 1):
        staged, table, totals, _ = decoded[ch]
        assert staged.size == int(totals[0]) + 64 * len(ALL)
        end = 0
        for name, e in zip(ALL, table):
            assert int(e["raw_offset"]) % 16 == 0 and int(e["raw_offset"]) >= end and int(e["out_offset"]) % 16 == 0
            end = int(e["raw_offset"]) + int(e["H"]) * (int(e["rowbytes"]) + 1)
            direct = png.is_direct(int(e["color_type"]), int(e["depth"]), ch)
            assert (int(e["work_offset"]) == -1) == direct and (int(e["pal_offset"]) >= end) == (int(e["color_type"]) == 3), name
        c = G.case("p8_2x5_trns")
        e = table[ALL.index("p8_2x5_trns")]
        pal = staged[int(e["pal_offset"]):int(e["pal_offset"]) + 1024].reshape(256, 4)
        assert np.array_equal(pal[:7, :3], c["palette"]) and not pal[7:].any() and not pal[:, 3].any()  # padded to 256 entries with zeros


def _with_ihdr(stream, **fields):
    chunks = PW.chunks_of(stream)
    W, H, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    v = dict(W=W, H=H, depth=depth, ct=ct, comp=comp, filt=filt, lace=lace)
    v.update(fields)
    chunks[0] = (b"IHDR", struct.pack(">IIBBBBB", v["W"], v["H"], v["depth"], v["ct"], v["comp"], v["filt"], v["lace"]))
    return PW.from_chunks(chunks)


def _refusals():
    c = G.case("rgb_3x5_idat7")
    rgb, good = c["samples"], G.write("rgb_2x2_ancillary")
    p = G.case("p2_65x5_f4")
    pal = lambda **kw: PW.write_png(p["samples"], 3, 2, 0, **kw)  # noqa: E731
    chunks = PW.chunks_of(PW.write_png(rgb, 2, 8, 0, idat_size=9))
    plte = (b"PLTE", bytes(12))
    scan = PW.filter_rows(PW.pack_rows(rgb, 8), 3, 0).tobytes()
    crc_at = len(good) - 12 - 4 - 1  # inside the CRC of the chunk before IEND
    return [
        ("Adam7 interlace", PW.write_png(rgb, 2, 8, 0, interlace=1)),
        ("16-bit samples", _with_ihdr(good, depth=16)),
        ("bit depth 4 is not allowed for colour type 2", _with_ihdr(good, depth=4)),
        ("bit depth 3 is not allowed", _with_ihdr(R.stream("g8_1x1_f0"), depth=3)),
        ("colour type 5", _with_ihdr(good, ct=5)),
        ("compression method 1", _with_ihdr(good, comp=1)),
        ("filter method 1", _with_ihdr(good, filt=1)),
        ("interlace method 2", _with_ihdr(good, lace=2)),
        ("zero or above", _with_ihdr(good, W=0)),
        ("zero or above", _with_ihdr(good, H=0)),
        ("zero or above", _with_ihdr(good, W=16385)),
        ("zero or above", _with_ihdr(good, H=1 << 31)),
        ("missing PLTE", pal()),
        ("PLTE is repeated", pal(palette=np.zeros((4, 3), np.uint8), before_idat=[plte])),
        ("oversized or malformed PLTE", pal(palette=np.zeros((5, 3), np.uint8))),
        ("oversized or malformed PLTE", PW.from_chunks([PW.chunks_of(pal())[0], (b"PLTE", bytes(7))] + PW.chunks_of(pal())[1:])),
        ("oversized or malformed PLTE", PW.write_png(rgb, 2, 8, 0, palette=np.zeros((257, 3), np.uint8))),
        ("PLTE follows IDAT", pal(after_idat=[plte])),
        ("IDAT chunks are not consecutive", PW.from_chunks(chunks[:2] + [(b"tEXt", b"k\0v")] + chunks[2:])),
        ("no IEND", PW.write_png(rgb, 2, 8, 0, end=False)),
        ("no IDAT", PW.from_chunks([chunks[0], chunks[-1]])),
        ("bad CRC", good[:crc_at] + bytes([good[crc_at] ^ 0x40]) + good[crc_at + 1:]),
        ("bad CRC", good[:17] + bytes([good[17] ^ 1]) + good[18:]),  # a changed IHDR byte
        ("zlib stream errors", PW.from_chunks([chunks[0], (b"IDAT", b"\x78\x9c" + bytes(range(40, 70))), chunks[-1]])),
        ("zlib stream errors", PW.from_chunks([chunks[0], (b"IDAT", zlib.compress(scan)[:-3]), chunks[-1]])),  # every pixel, but cut inside the checksum
        ("is only", PW.write_png(rgb, 2, 8, 0, scanlines=scan[:-1])),
        ("is only", PW.from_chunks([chunks[0], (b"IDAT", zlib.compress(scan)[:-8]), chunks[-1]])),  # cut inside the data
        ("is only 0 bytes", PW.write_png(rgb, 2, 8, 0, scanlines=b"")),
        ("is more than", PW.write_png(rgb, 2, 8, 0, scanlines=scan + b"\0")),
        ("is more than", PW.write_png(rgb, 2, 8, 0, scanlines=scan + bytes(1 << 22))),  # a stream that inflates far past its promise
        ("row 2 has filter type 5", PW.write_png(rgb, 2, 8, [0, 4, 5])),
        ("row 0 has filter type 255", PW.write_png(rgb, 2, 8, [255, 0, 0])),
        ("unknown critical chunk", PW.from_chunks(chunks[:1] + [(b"ABCD", b"x")] + chunks[1:])),
        ("IHDR is repeated", PW.from_chunks(chunks[:1] + chunks[:1] + chunks[1:])),
        ("first chunk is not a 13-byte IHDR", PW.from_chunks(chunks[1:])),
        ("signature", b"\x89PNG\r\n\x1a\r" + good[8:]),
        ("signature", b""),
        ("runs past the end", good[:33] + struct.pack(">I", 1 << 20) + good[37:]),
    ]


def test_every_refusal_names_its_clause_and_its_image(streams):
    cases = _refusals()
    assert len(cases) >= 30
    for clause, bad in cases:
        with pytest.raises(HpeError, match="image 1: .*" + clause):
            png.inflate_batch([streams[0], bad, streams[1]], 3, threads=2)
        with pytest.raises(HpeError, match="image 0: .*" + clause):
            png.inflate_batch([bad], 1, threads=1)
    # the lowest refused image is the one named, whatever the thread count
    for t in (1, 4):
        with pytest.raises(HpeError, match="image 1: .*Adam7"):
            png.inflate_batch([streams[0], cases[0][1], streams[1], cases[1][1]], 3, threads=t)
    with pytest.raises(HpeError, match="image 0: .*Adam7"):
        png.png_info(cases[0][1])
    # verify=False skips the CRCs only
    crc = [b for c, b in cases if c == "bad CRC"][0]
    png.inflate_batch([crc], 3, verify=False)
    with pytest.raises(ValueError):
        png.inflate_batch([], 3)
    with pytest.raises(ValueError):
        png.inflate_batch(streams[0], 3)
    with pytest.raises(ValueError, match="channels"):
        png.inflate_batch(streams, 2)


def test_inflate_is_capped_at_what_the_header_promises():
    """a deflate bomb behind a 3 x 5 header: zlib is asked for the promised size plus one byte, never for the stream's 4 MB"""
    import tracemalloc

    c = G.case("rgb_3x5_idat7")
    scan = PW.filter_rows(PW.pack_rows(c["samples"], 8), 3, 0).tobytes()
    bomb = PW.write_png(c["samples"], 2, 8, 0, scanlines=scan + bytes(1 << 22))
    assert len(bomb) < 8192
    tracemalloc.start()
    with pytest.raises(HpeError, match="more than"):
        png.inflate_batch([bomb], 3, threads=1)
    peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    assert peak < 1 << 20, peak


def test_every_prefix_of_the_smallest_colour_fixture_is_refused():
    s = R.stream(G.SMALLEST_COLOUR)
    for n in range(len(s)):
        with pytest.raises(HpeError, match="image 0: "):
            png.inflate_batch([s[:n]], 3, threads=1)
    png.inflate_batch([s], 3, threads=1)
    png.inflate_batch([s + b"trailing bytes after IEND"], 3, threads=1)


def test_ancillary_chunks_are_skipped(streams):
    kinds = [k for k, _ in PW.chunks_of(R.stream("rgb_2x2_ancillary"))]
    assert kinds == [b"IHDR", b"gAMA", b"acTL", b"IDAT", b"tEXt", b"IEND"]
    assert b"tRNS" in [k for k, _ in PW.chunks_of(R.stream("p8_2x5_trns"))]


def test_backend_refuses_a_damaged_table_before_any_launch(lib, streams):
    """hpe_png_backend holds every host table entry against the buffer sizes and against what H, W, colour type and depth imply; the
    check comes before the device pointers are looked at, so with NULL ones nothing can be launched and no GPU is needed"""
    names = ("p2_65x5_f4", "rgba_65x3_f3", "g8_65x67_cycle", "rgb_130x5_f4")
    _, table, totals = png.inflate_batch([R.stream(n) for n in names], 3, threads=1)
    table = table.copy()
    raw, ws, fr = (int(v) for v in totals[:3])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(t, raw=raw, ws=ws, fr=fr, B=len(names)):
        rc = lib.hpe_png_backend(p(t) if t is not None else None, None, B, None, raw, None, ws, None, fr, None)
        return rc, lib.hpe_last_error().decode()

    assert call(table) == (1, "null argument")  # a sound table: the NULL device pointers are what is refused
    assert call(None)[0] == 1 and call(table, B=0)[0] == 1 and call(table, raw=-1)[0] == 1
    assert [int(e["work_offset"]) for e in table] == [0, 144, 144 + 784, -1] and int(table[3]["store_group0"]) == int(totals[3])
    damage = [(0, "raw_offset", -16, "raw buffer"), (0, "raw_offset", 8, "raw buffer"), (3, "raw_offset", raw, "raw buffer"),
              (0, "pal_offset", -1, "palette"), (0, "pal_offset", raw - 1008, "palette"), (0, "pal_offset", int(table[0]["pal_offset"]) + 4, "palette"),
              (1, "pal_offset", 0, "pal_offset must be -1"),
              (1, "work_offset", ws, "workspace"), (1, "work_offset", -1, "workspace"), (2, "work_offset", 4, "workspace"),
              (3, "work_offset", 0, "direct"),
              (2, "out_offset", fr, "frame buffer"), (2, "out_offset", -16, "frame buffer"), (2, "out_offset", 8, "frame buffer"),
              (1, "H", 0, "H and W"), (1, "W", 16385, "H and W"), (1, "H", 16384, "raw buffer|workspace|frame buffer"),
              (1, "W", 4, "rowbytes"), (2, "rowbytes", 68, "rowbytes"), (0, "rowbytes", 1, "rowbytes"),
              (1, "color_type", 5, "colour type"), (1, "color_type", 2, "rowbytes"), (1, "depth", 4, "depth"), (1, "depth", 16, "depth"),
              (0, "depth", 3, "depth"), (1, "bpp", 3, "bpp"), (0, "bpp", 0, "bpp"), (1, "channels", 2, "channels"),
              (1, "store_group0", 0, "prefix sum"), (2, "store_group0", 1, "prefix sum"), (3, "store_group0", 0, "prefix sum")]
    for b, field, value, clause in damage:
        t = table.copy()
        t[b][field] = value
        rc, msg = call(t)
        assert rc == 1 and msg.startswith("table entry %d: " % b), (b, field, value, msg)
        assert re.search(clause, msg), (field, value, msg)
    for kw, clause in ((dict(raw=raw - 1), "table entry 0: .*palette|table entry 3: .*raw buffer"), (dict(ws=ws - 16), "table entry 2: .*workspace"),
                       (dict(fr=fr - 16), "table entry 3: .*frame buffer"), (dict(raw=0), "table entry 0"), (dict(fr=0), "table entry 0")):
        rc, msg = call(table, **kw)
        assert rc == 1 and re.search(clause, msg), (kw, msg)
