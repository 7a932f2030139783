"""CPU tests of the PNG encoder's definition (no GPU): the NumPy restatement of the filter rule and the chunk wrapping
(tests/png_encode_ref.py) produces streams that decode back to the input through the decoder's restatement (tests/png_ref.py, after
hpe_amd.png's host inflate) and through PIL where it is importable; across the shared cases every filter type is selected at least
once; an all-zero row ties on every candidate and takes filter 0; and the host half of hpe_amd.png_encode (table, chunk wrapping,
deflate on threads) agrees with the restatement."""
import numpy as np
import pytest

import hpe_amd
from hpe_amd import png, png_encode

import png_encode_ref as E
import png_ref as R

CASES = E.cases()


def decode_with_ref(stream, channels_of_frame):
    """chunk walk and inflate by hpe_amd.png (host), then the decoder's NumPy restatement -> the raw samples uint8 [H, W, C]"""
    staged, table, _ = png.inflate_batch([stream], 3 if channels_of_frame != 1 else 1, threads=1)
    e = table[0]
    H, W, rb, bpp = int(e["H"]), int(e["W"]), int(e["rowbytes"]), int(e["bpp"])
    o = int(e["raw_offset"])
    return R.unfilter(staged[o:o + H * (rb + 1)].reshape(H, rb + 1), bpp).reshape(H, W, bpp)


def test_the_shared_cases_are_the_issues_shapes():
    assert [f.shape for _, f in CASES] == E.SHAPES and all(f.dtype == np.uint8 for _, f in CASES)


@pytest.mark.parametrize("name,frame", CASES, ids=[n for n, _ in CASES])
def test_streams_decode_to_the_input(name, frame):
    s = E.encode(frame)
    info = hpe_amd.png_info(s)  # every CRC verified
    H, W, C = frame.shape
    assert (info["height"], info["width"], info["color_type"], info["depth"]) == (H, W, {1: 0, 3: 2, 4: 6}[C], 8)
    assert np.array_equal(decode_with_ref(s, C), frame)


@pytest.mark.parametrize("name,frame", CASES, ids=[n for n, _ in CASES])
def test_streams_decode_to_the_input_through_pil(name, frame):
    Image = pytest.importorskip("PIL.Image")
    import io

    got = np.asarray(Image.open(io.BytesIO(E.encode(frame))))
    assert np.array_equal(got.reshape(frame.shape), frame)


def test_every_filter_type_is_selected_at_least_once():
    chosen = np.concatenate([E.scanlines(f)[1] for _, f in CASES])
    assert set(chosen.tolist()) == {0, 1, 2, 3, 4}, np.bincount(chosen, minlength=5)


def test_an_all_zero_row_ties_and_takes_filter_0():
    f = np.zeros((3, 9, 3), np.uint8)
    assert (E.scores(E.candidates(f)) == 0).all()  # all five candidates score 0 on every row
    scan, ft = E.scanlines(f)
    assert ft.tolist() == [0, 0, 0] and not scan.any()
    g = np.zeros((2, 5, 1), np.uint8)
    g[0] = 77  # row 1 is zero under None (score 0); Up gives -77 everywhere: no tie, still 0
    assert E.scanlines(g)[1].tolist()[1] == 0


def test_hand_checked_row():
    """one RGB row 10 20 30 | 12 22 32: None scores 126, Sub 10+20+30+2+2+2 = 66, Up = None, Average 10+20+30+7+12+17 = 96, Paeth
    (no row above: the predictor is a) = Sub -> Sub wins over Paeth by the lower number"""
    f = np.array([[[10, 20, 30], [12, 22, 32]]], np.uint8)
    assert E.scores(E.candidates(f))[:, 0].tolist() == [126, 66, 126, 96, 66]
    scan, ft = E.scanlines(f)
    assert ft.tolist() == [1] and scan[0].tolist() == [1, 10, 20, 30, 2, 2, 2]


def test_host_half_agrees_with_the_restatement():
    """filter_table lays the scanlines out in batch order on 16-byte boundaries; deflate_batch on the restatement's scanlines gives the
    restatement's streams, whatever the thread count"""
    frames = [f for _, f in CASES]
    table, total = png_encode.filter_table([f.shape for f in frames], [0] * len(frames))
    assert table["row0"].tolist() == np.concatenate([[0], np.cumsum([f.shape[0] for f in frames])[:-1]]).tolist()
    assert all(o % 16 == 0 for o in table["scan_offset"].tolist()) and total % 16 == 0
    host = np.zeros(total, np.uint8)
    for e, f in zip(table, frames):
        s = E.scanlines(f)[0].reshape(-1)
        host[int(e["scan_offset"]):int(e["scan_offset"]) + s.size] = s
    one = png_encode.deflate_batch(host, table, threads=1)
    assert one == [E.encode(f) for f in frames]
    assert png_encode.deflate_batch(host, table, threads=5) == one
    assert png_encode.deflate_batch(host, table, level=1, threads=2) == [E.encode(f, 1) for f in frames]


def test_arguments_are_checked_without_a_device():
    with pytest.raises(ValueError, match="threads"):
        png_encode.deflate_batch(np.zeros(16, np.uint8), png_encode.filter_table([(1, 1, 1)], [0])[0], threads=17)
    with pytest.raises(ValueError, match="level"):
        png_encode.deflate_batch(np.zeros(16, np.uint8), png_encode.filter_table([(1, 1, 1)], [0])[0], level=10)
    with pytest.raises(ValueError, match="frames must be"):
        hpe_amd.encode_png_batch(np.zeros((1, 2, 2, 3), np.uint8))


def test_filter_call_checks_its_table_before_any_device_is_needed():
    """hpe_png_filter checks the host table first: every refusal below comes back without a GPU"""
    import ctypes as C

    from hpe_amd import _lib

    lib = _lib.load()

    def call(shape, frames_bytes=1 << 20, scan_bytes=1 << 20, row0=0, B=1, table=True):
        t = np.zeros(1, png_encode.FILTER_DTYPE)
        t[0] = (0, 0) + shape + (row0,)
        rc = lib.hpe_png_filter(t.ctypes.data_as(C.c_void_p) if table else None, None, B, None, frames_bytes, None, scan_bytes, None)
        return rc, lib.hpe_last_error().decode()

    assert call((4, 4, 2)) == (1, "table entry 0: C must be 1, 3 or 4")
    assert call((0, 4, 3))[1].endswith("H and W must be in [1, 16384]") and call((4, 16385, 3))[0] == 1
    assert "outside the frame buffer" in call((4, 4, 3), frames_bytes=47)[1]
    assert "outside the scanline buffer" in call((4, 4, 3), scan_bytes=51)[1]
    assert "row base" in call((4, 4, 3), row0=1)[1]
    assert call((4, 4, 3), B=0) == (1, "B must be >= 1") and call((4, 4, 3), table=False) == (1, "null argument")
    assert call((4, 4, 3), frames_bytes=48, scan_bytes=52) == (1, "null argument")  # a sound table: the NULL device pointers are next
