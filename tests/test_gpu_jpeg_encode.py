"""GPU tests of the JPEG encoder (run with -m gpu on an MI355X).  Every comparison is exact equality -- the contract has no tolerance:
the coefficients of ``forward_dct_batch`` against ``entropy_decode`` of the streams Pillow's libjpeg-turbo wrote of the same pixels
(tests/golden/make_jpeg_encode_golden.py), element for element with the dummy blocks, as one mixed batch, singly and in reverse; that
nothing outside the images' planes is written; two calls and two graph replays to the same bits; ``encode_jpeg_batch`` against the
golden streams byte for byte for every input form; the round trip through the decoder; the refusals."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, batch_io, jpeg, jpeg_encode

import jpeg_encode_ref as R

pytestmark = pytest.mark.gpu
NAMES = tuple(R.CASES)
assert len(NAMES) == 12
SETTINGS = sorted({R.CASES[n][3:] for n in NAMES})  # (quality, subsampling): one call takes one setting


@pytest.fixture(scope="module")
def want():
    """name -> the int16 coefficients of Pillow's stream, all planes back to back in component order"""
    out = {}
    for n in NAMES:
        coef, table, _ = jpeg.entropy_decode([R.stream(n)], R.CASES[n][2])
        assert int(table[0]["ncomp"]) == R.CASES[n][2]
        coef.setflags(write=False)
        out[n] = coef
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def groups(names):
    """the fixtures of ``names`` that share a (quality, subsampling), in the order given; a grey frame goes with any sampling"""
    for q, sub in SETTINGS:
        part = [n for n in names if R.CASES[n][3] == q and (R.CASES[n][4] == sub or R.CASES[n][2] == 1)]
        if part:
            yield q, sub, part


def assert_coefficients(names, want, guard=64):
    for q, sub, part in groups(names):
        frames = [dev(R.pixels(n)) for n in part]
        n_coef = sum(want[n].size for n in part)
        out = torch.full((guard + n_coef + guard + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
        coef, table = jpeg_encode.forward_dct_batch(frames, q, sub, out=out[guard:guard + n_coef + 8])
        host = out.cpu().numpy()
        assert (host[:guard] == 0x5A5A).all() and (host[guard + n_coef:] == 0x5A5A).all(), "a guard element was written"
        pos = 0
        for b, (n, e) in enumerate(zip(part, table)):
            assert int(e["coef_offset"][0]) == pos
            got = host[guard + pos:guard + pos + want[n].size]
            diff = got != want[n]
            assert not diff.any(), "%s (image %d of q %d %s): %d coefficients differ, first at %d" % (n, b, q, sub, int(diff.sum()), int(np.argmax(diff)))
            pos += want[n].size


def test_mixed_batches_equal_pillows_coefficients(want):
    assert_coefficients(NAMES, want)
    assert_coefficients(NAMES[::-1], want)


def test_each_fixture_alone_equals_pillows_coefficients(want):
    for n in NAMES:
        assert_coefficients([n], want)


def test_every_fixture_was_compared(want):
    seen = [n for _, _, part in groups(NAMES) for n in part]
    assert set(seen) == set(NAMES)


def test_gaps_between_images_keep_their_bytes_and_two_calls_agree(want):
    """a hand-laid table with 192 unused elements between the images' planes: they keep 0x5A5A; a second call gives the same bits"""
    part = ["rgb_17x33", "rgb_8x24", "rgb_3x5"]
    frames = [dev(R.pixels(n)) for n in part]
    buf, shapes, offsets = batch_io.pack_frames(frames, jpeg_encode.CHANNELS)
    table, totals = jpeg_encode.encode_layout(shapes, offsets, 95, "4:2:0")
    gap = 192
    for b in range(len(part)):
        table[b]["coef_offset"] += gap * (b + 1)
    n = int(totals[0]) + gap * (len(part) + 1)
    lib = _lib.load()
    table_dev = dev(table.view(np.uint8))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = []
    for _ in range(2):
        out = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
        _lib.check(lib.hpe_jpeg_forward(table.ctypes.data_as(C.c_void_p), table_dev.data_ptr(), len(part), buf.data_ptr(), buf.numel(), out.data_ptr(), n, st))
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    written = np.zeros(n, bool)
    for name, e in zip(part, table):
        o = int(e["coef_offset"][0])
        assert np.array_equal(runs[0][o:o + want[name].size], want[name]), name
        written[o:o + want[name].size] = True
    assert int((~written).sum()) == gap * (len(part) + 1) and (runs[0][~written] == 0x5A5A).all()


def test_launch_replays_from_a_graph(want):
    part = [n for n in NAMES if R.CASES[n][3:] == (95, "4:2:0")]
    buf, shapes, offsets = batch_io.pack_frames([dev(R.pixels(n)) for n in part], jpeg_encode.CHANNELS)
    table, totals = jpeg_encode.encode_layout(shapes, offsets, 95, "4:2:0")
    table_dev = dev(table.view(np.uint8))
    coef = torch.zeros(int(totals[0]), dtype=torch.int16, device="cuda")
    lib = _lib.load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.hpe_jpeg_forward(table.ctypes.data_as(C.c_void_p), table_dev.data_ptr(), len(part), buf.data_ptr(), buf.numel(), coef.data_ptr(),
                                        coef.numel(), st))
    expect = np.concatenate([want[n] for n in part])
    for _ in range(2):
        coef.fill_(0x5A5A)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(coef.cpu().numpy(), expect)


def test_encode_returns_the_golden_streams_for_every_input_form():
    for q, sub, part in groups(NAMES):
        got = hpe_amd.encode_jpeg_batch([dev(R.pixels(n)) for n in part], quality=q, subsampling=sub, threads=3)
        for n, s in zip(part, got):
            assert s == R.stream(n), "%s: %d bytes, Pillow wrote %d" % (n, len(s), len(R.stream(n)))
    px = R.pixels("rgb_8x24")
    assert hpe_amd.encode_jpeg_batch(dev(np.stack([px, px]))) == [R.stream("rgb_8x24")] * 2  # [B,H,W,C]
    mask = R.pixels("mask_37x43")
    assert hpe_amd.encode_jpeg_batch(dev(mask[None])) == [R.stream("mask_37x43")]  # [B,H,W]
    assert hpe_amd.encode_jpeg_batch(dev(mask[None, :, :, None])) == [R.stream("mask_37x43")]  # [B,H,W,1]
    batch = hpe_amd.decode_png_batch(hpe_amd.encode_png_batch([dev(R.pixels("rgb_17x33")), dev(R.pixels("rgb_3x5"))]), channels=3)
    assert hpe_amd.encode_jpeg_batch(batch) == [R.stream("rgb_17x33"), R.stream("rgb_3x5")]  # a DecodedBatch goes in as it is
    one = hpe_amd.encode_jpeg_batch(batch, threads=1)
    assert hpe_amd.encode_jpeg_batch(batch, threads=16) == one
    assert hpe_amd.encode_jpeg_batch(batch, density=(72, 96, "cm"))[0][13:18] == bytes([2, 0, 72, 0, 96])


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:2", "4:2:0"])
def test_encode_equals_pillow_today(sub):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState({"4:4:4": 444, "4:2:2": 422, "4:2:0": 420}[sub])
    frames = [np.clip(rng.normal(128, 60, (h, w, 3)), 0, 255).astype(np.uint8) for h, w in ((40, 56), (23, 9), (8, 8))]
    got = hpe_amd.encode_jpeg_batch([dev(f) for f in frames], quality=77, subsampling=sub)
    for f, s in zip(frames, got):
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, "JPEG", quality=77, subsampling=sub, dpi=(300, 300))
        assert s == buf.getvalue()


def test_round_trip_through_the_decoder(want):
    for q, sub, part in groups(NAMES):
        frames = [dev(R.pixels(n)) for n in part]
        back = hpe_amd.decode_jpeg_batch(hpe_amd.encode_jpeg_batch(frames, quality=q, subsampling=sub), channels=3)
        for n, f in zip(part, back.frames):
            d = R.decoded(n)
            d = d if d.ndim == 3 else np.repeat(d[:, :, None], 3, axis=2)
            assert np.array_equal(f.cpu().numpy(), d), n
        # the device coefficient buffer as it stands, straight into the decoder's back end
        coef, enc = jpeg_encode.forward_dct_batch(frames, q, sub)
        _, table, totals = jpeg.entropy_decode([R.stream(n) for n in part], channels=3)
        assert all(np.array_equal(table["coef_offset"][b][:int(enc[b]["C"])], enc["coef_offset"][b][:int(enc[b]["C"])]) for b in range(len(part)))
        table_dev = dev(table.view(np.uint8))
        workspace = torch.empty(int(totals[1]), dtype=torch.uint8, device="cuda")
        out = torch.zeros(int(totals[2]), dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.load().hpe_jpeg_backend(table.ctypes.data_as(C.c_void_p), table_dev.data_ptr(), len(part), coef.data_ptr(), coef.numel(),
                                                workspace.data_ptr(), workspace.numel(), out.data_ptr(), out.numel(), st))
        direct = jpeg.DecodedBatch(out, back.sizes, table["out_offset"].astype(np.int64), 3)
        assert all(torch.equal(a, b) for a, b in zip(direct.frames, back.frames))


def test_refusals_name_the_image_and_launch_nothing():
    ok = dev(np.zeros((4, 4, 3), np.uint8))
    for bad, clause in ((torch.zeros(4, 4, 3, dtype=torch.uint8), "image 1: the frame is not on a CUDA device"),
                        (dev(np.zeros((4, 4, 3), np.float32)), "image 1: dtype float32"),
                        (dev(np.zeros((4, 4, 4), np.uint8)), "image 1: 4 channels"),
                        (dev(np.zeros((0, 4, 3), np.uint8)), "image 1: an empty side"),
                        (dev(np.zeros((1, 16385, 1), np.uint8)), "image 1: a side of")):
        with pytest.raises(hpe_amd.HpeError, match=clause):
            hpe_amd.encode_jpeg_batch([ok, bad])
        out = torch.full((4096,), 0x5A5A, dtype=torch.int16, device="cuda")
        with pytest.raises(hpe_amd.HpeError, match=clause):
            jpeg_encode.forward_dct_batch([ok, bad], out=out)
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A).all()), clause
    with pytest.raises(hpe_amd.HpeError, match="image 0: 4 channels"):
        hpe_amd.encode_jpeg_batch(dev(np.zeros((2, 4, 4, 4), np.uint8)))
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="4:1:1"), dict(threads=0), dict(threads=17), dict(density=(300, 300, "m"))):
        with pytest.raises(hpe_amd.HpeError):
            hpe_amd.encode_jpeg_batch([ok], **kw)


def test_forward_refusals_leave_the_output_untouched():
    """a frame past the frame buffer, coefficients past the coefficient buffer, a wrong grid, a wrong workgroup base, a NULL pointer:
    HPE_ERR_INVALID and not one element written"""
    lib = _lib.load()
    frames = dev(np.full(9 * 11 * 3, 9, np.uint8))
    coef = torch.full((1024,), 0x5A5A, dtype=torch.int16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base, totals = jpeg_encode.encode_layout([(9, 11, 3)], None, 95, "4:2:0")
    assert int(totals[0]) == 64 * 6

    def call(edit=None, frames_ptr=None, frames_bytes=9 * 11 * 3, coef_count=1024):
        t = base.copy()
        if edit:
            edit(t[0])
        td = dev(t.view(np.uint8))
        rc = lib.hpe_jpeg_forward(t.ctypes.data_as(C.c_void_p), td.data_ptr(), 1, frames.data_ptr() if frames_ptr is None else frames_ptr, frames_bytes,
                                  coef.data_ptr(), coef_count, st)
        torch.cuda.synchronize()
        return rc, lib.hpe_last_error().decode()

    def set_field(name, value, index=None):
        def edit(e):
            if index is None:
                e[name] = value
            else:
                e[name][index] = value
        return edit

    assert call()[0] == 0 and int((coef.cpu() != 0x5A5A).sum()) > 0 and bool((coef[384:].cpu() == 0x5A5A).all())
    coef.fill_(0x5A5A)
    for kw, clause in ((dict(frames_bytes=9 * 11 * 3 - 1), "outside the frame buffer"), (dict(coef_count=383), "outside the coefficient buffer"),
                       (dict(edit=set_field("blocks_w", 3, 0)), "block grid"), (dict(edit=set_field("real_h", 1, 0)), "real block grid"),
                       (dict(edit=set_field("group0", 1)), "workgroup base"), (dict(edit=set_field("C", 4)), "C must be 1 or 3"),
                       (dict(edit=set_field("W", 16385)), "H and W"), (dict(edit=set_field("coef_offset", 4, 1)), "8-element boundary"),
                       (dict(frames_ptr=0), "null argument")):
        rc, msg = call(**kw)
        assert rc == 1 and clause in msg, (kw, rc, msg)
        assert bool((coef.cpu() == 0x5A5A).all()), kw
