"""The host half of the JPEG encoder without a GPU.  The NumPy restatement (tests/jpeg_encode_ref.py) stands in for the launch: its
coefficients through the library's entropy coder (hpe_jpeg_entropy_encode) equal, byte for byte and header included, the streams
Pillow's libjpeg-turbo wrote when the fixtures were made (tests/golden/make_jpeg_encode_golden.py), and equal what the library's own
decoder reads back from those streams, dummy blocks included.  The bytes do not depend on the thread count; what the decoder reads from
its own 14 fixtures codes and decodes again to the same coefficients; no write leaves the caller's buffer; everything out of range is
refused.  There is no tolerance anywhere."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_encode_ref as R
import jpeg_ref as JR
from hpe_amd import HpeError, _lib, build as hbuild, jpeg, jpeg_encode as JE

NAMES = tuple(R.CASES)


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


@pytest.fixture(scope="module")
def restated(lib):
    """name -> (the restatement's coefficients, the library's table entry), computed once"""
    out = {}
    for n, (H, W, Cn, q, sub) in R.CASES.items():
        coef, _ = R.forward([R.pixels(n)], q, sub)
        table, totals = JE.encode_layout([(H, W, Cn)], None, q, sub)
        assert int(totals[0]) == coef.size
        coef.setflags(write=False)
        out[n] = (coef, table)
    return out


def test_there_are_twelve_fixtures_each_under_the_size_limit():
    assert len(NAMES) == 12
    for n, (H, W, Cn, _, _) in R.CASES.items():
        assert R.pixels(n).shape == ((H, W, 3) if Cn == 3 else (H, W)) and len(R.stream(n)) < 6144


@pytest.mark.parametrize("name", NAMES)
def test_restatement_through_the_entropy_coder_equals_the_golden_stream(restated, name):
    coef, table = restated[name]
    got = JE.entropy_encode(coef, table, threads=1)[0]
    want = R.stream(name)
    assert got == want, "%d bytes, Pillow wrote %d; first difference at %d" % (
        len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))
    assert R.encode(R.pixels(name), *R.CASES[name][3:]) == want  # the restatement's own coder as well


@pytest.mark.parametrize("name", NAMES)
def test_restatement_coefficients_equal_the_decoded_golden_stream(restated, name):
    coef, table = restated[name]
    got, dec, _ = jpeg.entropy_decode([R.stream(name)], R.CASES[name][2])
    assert np.array_equal(got, coef), "%d coefficients differ" % int((got != coef).sum())
    e, d = table[0], dec[0]
    n = int(e["C"])
    assert (int(d["H"]), int(d["W"]), int(d["ncomp"]), int(d["hmax"]), int(d["vmax"])) == (int(e["H"]), int(e["W"]), n, int(e["hmax"]), int(e["vmax"]))
    for f in ("coef_offset", "blocks_w", "blocks_h"):
        assert np.array_equal(d[f][:n], e[f][:n]), f
    assert all(np.array_equal(d["quant"][c], e["quant"][min(c, 1)]) for c in range(n))


def test_the_fixtures_reach_their_rules(restated):
    dummy = {n: any(int(t[0]["real_w"][c]) < int(t[0]["blocks_w"][c]) or int(t[0]["real_h"][c]) < int(t[0]["blocks_h"][c]) for c in range(int(t[0]["C"])))
             for n, (_, t) in restated.items()}
    assert dummy["rgb_1x1"] and dummy["rgb_3x5"] and dummy["rgb_8x24"] and dummy["rgb_17x33"] and not dummy["grey_9x11"]
    e = restated["rgb_17x33"][1][0]  # right AND bottom dummies: the corner's DC chains through a dummy
    assert (int(e["real_w"][0]), int(e["blocks_w"][0]), int(e["real_h"][0]), int(e["blocks_h"][0])) == (5, 6, 3, 4)
    assert R.CASES["rgb_8x24"][0] % 16 == 8
    coef = restated["noise_q30_24x40"][0].reshape(-1, 64)[:, R.ZIGZAG]
    longest = max(int(np.diff(np.concatenate([[0], np.nonzero(b[1:])[0] + 1])).max(initial=0)) for b in coef)
    assert longest > 16, "no run of 16 zeros before a coefficient: ZRL is not reached"
    assert JE.quant_tables(1).max() == 255 and JE.quant_tables(100).max() == 1 and JE.quant_tables(95)[0][0] == 2
    e = restated["ramp_q85_97x130"][1][0]
    assert int(e["blocks_w"][0]) * int(e["blocks_h"][0]) == 252 and 252 % 32  # several workgroups, and one that spans two components


@pytest.mark.parametrize("quality", [1, 30, 49, 50, 75, 95, 100])
def test_quant_tables_equal_the_restatement(lib, quality):
    assert np.array_equal(JE.quant_tables(quality), R.quant_tables(quality))


def test_mixed_batch_and_thread_counts_give_the_same_bytes(restated):
    """all twelve in ONE coefficient buffer, coded on 1 and on 4 threads"""
    parts, tables, pos = [], [], 0
    for n in NAMES:
        coef, table = restated[n]
        t = table.copy()
        t["coef_offset"][0][:int(t[0]["C"])] += pos
        parts.append(coef)
        tables.append(t)
        pos += coef.size
    coef, table = np.concatenate(parts), np.concatenate(tables)
    one = JE.entropy_encode(coef, table, threads=1)
    assert one == [R.stream(n) for n in NAMES]
    assert JE.entropy_encode(coef, table, threads=4) == one and JE.entropy_encode(coef, table, threads=16) == one


@pytest.mark.parametrize("name", JR.CASES)
def test_decoder_fixtures_code_and_decode_to_the_same_coefficients(lib, name):
    """the 14 decoder fixtures (optimised tables, restart markers, other qualities among them): decoded, coded with the standard tables,
    decoded again"""
    coef, table, _ = jpeg.entropy_decode([JR.stream(name)], 3)
    again = JE.entropy_encode(coef, JE.table_from_decoded(table))[0]
    coef2, table2, _ = jpeg.entropy_decode([again], 3)
    assert np.array_equal(coef2, coef)
    assert table2.tobytes() == table.tobytes()


def test_capacity_bound_holds_and_a_short_buffer_is_refused_with_its_canaries(lib, restated):
    for n in NAMES + ("worst",):
        if n == "worst":  # every AC term at the largest magnitude the tables code, DC alternating: the longest codes there are
            table, totals = JE.encode_layout([(16, 16, 3)], None, 100, "4:2:0")
            coef = np.full(int(totals[0]), 1023, np.int16)
            coef[1::2] = -1023
            coef[0::64] = np.where(np.arange(coef.size // 64) % 2, -1023, 1023)
        else:
            coef, table = restated[n]
        bound = int(JE.stream_bound(table).sum())
        buf = np.full(bound + 32, 0xC3, np.uint8)
        streams = JE.entropy_encode(coef, table, out=buf[16:16 + bound])
        assert len(streams[0]) <= bound and (buf[:16] == 0xC3).all() and (buf[16 + bound:] == 0xC3).all(), n
        again, _, _ = jpeg.entropy_decode(streams, int(table[0]["C"]))
        assert np.array_equal(again, coef), n
        buf[:] = 0xC3
        with pytest.raises(HpeError, match="out_capacity %d is below the batch's bound %d" % (bound - 1, bound)):
            JE.entropy_encode(coef, table, out=buf[16:16 + bound - 1])
        assert (buf == 0xC3).all(), n


def test_uncodable_coefficients_are_refused_by_image(lib, restated):
    coef, table = restated["grey_9x11"]
    for index, value in ((5, 1024), (5, -1024), (0, 2048), (64, -3000)):
        bad = coef.copy()
        bad[index] = value
        with pytest.raises(HpeError, match="image 0: a coefficient the standard Huffman tables cannot code"):
            JE.entropy_encode(bad, table)


def test_out_of_range_arguments_are_refused(lib, restated):
    for q in (0, 101, -5, 95.5):
        with pytest.raises(HpeError, match="quality"):
            JE.encode_layout([(8, 8, 3)], None, q)
    for sub in ("4:1:1", "420", None):
        with pytest.raises(HpeError, match="subsampling"):
            JE.encode_layout([(8, 8, 3)], None, 95, sub)
    for shape, clause in (((8, 8, 4), "image 1: 4 channels"), ((8, 8, 2), "image 1: 2 channels"), ((0, 8, 3), "image 1: an empty side"),
                          ((8, 16385, 1), "image 1: a side of")):
        with pytest.raises(HpeError, match=clause):
            JE.encode_layout([(8, 8, 3), shape])
    coef, table = restated["rgb_3x5"]
    for t in (0, 17, 2.5):
        with pytest.raises(HpeError, match="threads"):
            JE.entropy_encode(coef, table, threads=t)
    for d in ((300, 300, "furlong"), (0, 300, "in"), (300, 65536, "in"), (300, 300)):
        with pytest.raises(HpeError, match="density"):
            JE.entropy_encode(coef, table, density=d)
    # the C ABI itself: the checks do not rest on the Python wrapper
    offsets, lengths, out = np.zeros(1, np.int64), np.zeros(1, np.int64), np.full(4096, 0xC3, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(table, threads=1, units=1, xd=300, coef_count=coef.size):
        return lib.hpe_jpeg_entropy_encode(p(table), 1, p(coef), coef_count, units, xd, 300, threads, p(out), out.size, p(offsets), p(lengths))

    assert call(table) == 0 and int(lengths[0]) == len(R.stream("rgb_3x5"))
    out[:] = 0xC3
    bad_grid, bad_c, bad_q = table.copy(), table.copy(), table.copy()
    bad_grid[0]["blocks_w"][0] = 4
    bad_c[0]["C"] = 2
    bad_q[0]["quant"][1][63] = 0
    for kw, clause in ((dict(table=table, threads=0), "threads"), (dict(table=table, threads=17), "threads"), (dict(table=table, units=3), "units"),
                       (dict(table=table, xd=0), "densities"), (dict(table=table, coef_count=coef.size - 1), "outside the coefficient buffer"),
                       (dict(table=bad_grid), "block grid"), (dict(table=bad_c), "C must be 1 or 3"), (dict(table=bad_q), "entry of 0")):
        assert call(**kw) == 1 and clause in lib.hpe_last_error().decode(), kw
        assert (out == 0xC3).all(), kw
    sh, off, tab, tot = np.array([[8, 8, 3]], np.int32), np.zeros(1, np.int64), np.zeros(1, JE.ENC_DTYPE), np.zeros(3, np.int64)
    assert lib.hpe_jpeg_encode_layout(1, p(sh), p(off), 2, 2, 95, p(tab), p(tot)) == 0
    assert lib.hpe_jpeg_encode_layout(1, p(sh), p(off), 1, 2, 95, p(tab), p(tot)) == 1 and b"sampling" in lib.hpe_last_error()
    assert lib.hpe_jpeg_encode_layout(1, p(sh), p(off), 2, 2, 0, p(tab), p(tot)) == 1 and b"quality" in lib.hpe_last_error()
    assert lib.hpe_jpeg_encode_layout(0, p(sh), p(off), 2, 2, 95, p(tab), p(tot)) == 1


def test_forward_checks_its_table_without_a_device(lib, restated):
    """hpe_jpeg_forward holds the host table against the buffer sizes before it looks at a device pointer"""
    _, table = restated["rgb_17x33"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n_frame, n_coef = 17 * 33 * 3, 64 * (24 + 6 + 6)
    assert lib.hpe_jpeg_forward(p(table), None, 1, None, n_frame, None, n_coef, None) == 1 and b"null argument" in lib.hpe_last_error()
    assert lib.hpe_jpeg_forward(p(table), None, 1, None, n_frame - 1, None, n_coef, None) == 1 and b"outside the frame buffer" in lib.hpe_last_error()
    assert lib.hpe_jpeg_forward(p(table), None, 1, None, n_frame, None, n_coef - 1, None) == 1 and b"outside the coefficient buffer" in lib.hpe_last_error()


@pytest.mark.parametrize("name", NAMES)
def test_goldens_equal_pillow_today(name):
    Image = pytest.importorskip("PIL.Image")
    H, W, Cn, q, sub = R.CASES[name]
    buf = io.BytesIO()
    args = dict(subsampling=sub) if Cn == 3 else {}
    Image.fromarray(R.pixels(name)).save(buf, "JPEG", quality=q, dpi=(300, 300), **args)
    assert buf.getvalue() == R.stream(name)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(R.stream(name)))), R.decoded(name))
