"""GPU tests of the PNG encoder (run with -m gpu on an MI355X): the scanlines of ``hpe_png_filter`` against the NumPy restatement
(tests/png_encode_ref.py) byte for byte -- the contract has no tolerance -- on the shared cases in one mixed batch and singly, on a
65536-byte row and on a 672 x 672 x 3 panel; ``decode_png_batch(encode_png_batch(x))`` against x; the refusals, each leaving the
output untouched; that the bytes do not depend on the thread count; and the launch replayed from a captured graph."""
import ctypes as C

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, batch_io, jpeg_encode, png, png_encode

import png_encode_ref as E
import png_ref as R

pytestmark = pytest.mark.gpu
CASES = E.cases()


@pytest.fixture(scope="module")
def want():
    """the restatement's scanlines of every shared case, computed once"""
    return {n: E.scanlines(f)[0] for n, f in CASES}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_scanlines(frames, wants):
    scan, table = png_encode.filter_batch([dev(f) for f in frames])
    host = scan.cpu().numpy()
    end = 0
    for b, (e, w) in enumerate(zip(table, wants)):
        o = int(e["scan_offset"])
        assert not host[end:o].any(), "padding before image %d was written" % b
        got = host[o:o + w.size].reshape(w.shape)
        diff = got != w
        assert not diff.any(), "image %d %s: %d bytes differ, first at %s (filters got %s want %s)" % (
            b, frames[b].shape, int(diff.sum()), np.argwhere(diff)[0].tolist(), got[:, 0].tolist()[:8], w[:, 0].tolist()[:8])
        end = o + w.size
    assert not host[end:].any()


def test_mixed_batch_equals_the_restatement(want):
    assert_scanlines([f for _, f in CASES], [want[n] for n, _ in CASES])
    assert_scanlines([f for _, f in CASES[::-1]], [want[n] for n, _ in CASES[::-1]])


def test_single_image_batches_equal_the_restatement(want):
    for n, f in CASES:
        assert_scanlines([f], [want[n]])


def test_grey_frames_without_a_channel_axis(want):
    n, f = CASES[4]  # 5 x 7 x 1
    assert_scanlines([f[:, :, 0]], [want[n]])


def test_a_row_of_65536_bytes():
    f = E.content(2, 16384, 4, seed=3)
    f[1, 100:9000] = np.random.RandomState(5).randint(0, 256, (8900, 4))
    assert_scanlines([f], [E.scanlines(f)[0]])


def test_a_672_panel():
    f = E.content(672, 672, 3, seed=1)
    assert_scanlines([f], [E.scanlines(f)[0]])


def test_batch_tensor_and_decoded_batch_inputs(want):
    x = np.stack([E.content(6, 5, 3, seed=s) for s in range(3)])
    scan, table = png_encode.filter_batch(dev(x))
    host = scan.cpu().numpy()
    for e, f in zip(table, x):
        w = E.scanlines(f)[0]
        assert np.array_equal(host[int(e["scan_offset"]):int(e["scan_offset"]) + w.size].reshape(w.shape), w)
    streams = hpe_amd.encode_png_batch(dev(x))
    batch = hpe_amd.decode_png_batch(streams, channels=3)
    again = hpe_amd.encode_png_batch(batch)  # a DecodedBatch goes in as it is
    assert again == streams


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_decode_of_encode_is_the_input(channels):
    """decode_png_batch returns 1 or 3 channels: grey and RGB come back whole; of RGBA it returns the colour (alpha is dropped, DESIGN.md
    "PNG streams in the records"), so the alpha plane is held against the stream's unfiltered rows (host inflate + tests/png_ref.py)"""
    frames = [E.content(h, w, channels, seed=h) for h, w in ((1, 1), (7, 3), (33, 65), (70, 9))]
    streams = hpe_amd.encode_png_batch([dev(f) for f in frames], threads=2)
    assert all(s == E.encode(f) for s, f in zip(streams, frames))  # the same filters, the same zlib: the same bytes
    batch = hpe_amd.decode_png_batch(streams, channels=1 if channels == 1 else 3)
    for got, f in zip(batch.frames, frames):
        got = got.cpu().numpy()
        assert np.array_equal(got.reshape(f.shape[0], f.shape[1], -1), f[:, :, :3])
    if channels == 4:
        staged, table, _ = png.inflate_batch(streams, 3, threads=1)
        for e, f in zip(table, frames):
            H, rb, o = int(e["H"]), int(e["rowbytes"]), int(e["raw_offset"])
            assert np.array_equal(R.unfilter(staged[o:o + H * (rb + 1)].reshape(H, rb + 1), 4).reshape(f.shape), f)


def test_bytes_do_not_depend_on_threads():
    frames = [dev(f) for _, f in CASES]
    one = hpe_amd.encode_png_batch(frames, threads=1)
    assert hpe_amd.encode_png_batch(frames, threads=7) == one and hpe_amd.encode_png_batch(frames, threads=16) == one
    assert hpe_amd.encode_png_batch(frames, level=1) != one


def test_encode_refuses_with_the_image_and_the_clause():
    ok = dev(np.zeros((4, 4, 3), np.uint8))
    for bad, clause in ((dev(np.zeros((4, 4, 2), np.uint8)), "image 1: 2 channels"),
                        (dev(np.zeros((4, 4, 3), np.float32)), "image 1: dtype float32"),
                        (dev(np.zeros((0, 4, 3), np.uint8)), "image 1: an empty side"),
                        (dev(np.zeros((1, 16385, 1), np.uint8)), "image 1: a side of"),
                        (torch.zeros(4, 4, 3, dtype=torch.uint8), "image 1: the frame is not on a CUDA device")):
        with pytest.raises(hpe_amd.HpeError, match=clause):
            hpe_amd.encode_png_batch([ok, bad])
    with pytest.raises(hpe_amd.HpeError, match="image 0: 2 channels"):
        hpe_amd.encode_png_batch(dev(np.zeros((2, 4, 4, 2), np.uint8)))


def test_filter_refusals_leave_the_output_untouched():
    """C = 2, an empty side, a side above the maximum, a NULL pointer, a short output buffer: HPE_ERR_INVALID, and not one byte written"""
    lib = _lib.load()
    frames = dev(np.full(4 * 4 * 4, 9, np.uint8))
    scan = torch.full((256,), 0xA5, dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(shape, frames_ptr=None, scan_bytes=256, frames_bytes=64):
        t = np.zeros(1, png_encode.FILTER_DTYPE)
        t[0] = (0, 0) + shape + (0,)
        td = dev(t.view(np.uint8))
        rc = lib.hpe_png_filter(t.ctypes.data_as(C.c_void_p), td.data_ptr(), 1, frames.data_ptr() if frames_ptr is None else frames_ptr, frames_bytes,
                                scan.data_ptr(), scan_bytes, st)
        torch.cuda.synchronize()
        return rc, lib.hpe_last_error().decode()

    assert call((4, 4, 3))[0] == 0 and int((scan.cpu() != 0xA5).sum()) == 4 * 13  # the sound call writes exactly its scanlines
    scan.fill_(0xA5)
    for kw, clause in ((dict(shape=(4, 4, 2)), "C must be 1, 3 or 4"), (dict(shape=(0, 4, 3)), "H and W"), (dict(shape=(4, 16385, 1), frames_bytes=1 << 20, scan_bytes=1 << 20), "H and W"),
                       (dict(shape=(4, 4, 3), frames_ptr=0), "null argument"), (dict(shape=(4, 4, 3), scan_bytes=51), "outside the scanline buffer")):
        rc, msg = call(**kw)
        assert rc == 1 and clause in msg, (kw, rc, msg)
        assert bool((scan.cpu() == 0xA5).all()), kw


def test_filter_launch_replays_from_a_graph(want):
    """hpe_png_filter captured on one stream and replayed twice: the restatement's scanlines again, after the output was wiped"""
    frames = [f for _, f in CASES]
    buf, shapes, offsets = batch_io.pack_frames([dev(f) for f in frames], png_encode.COLOR_TYPE)
    table, scan_bytes = png_encode.filter_table(shapes, offsets)
    table_dev = dev(table.view(np.uint8))
    scan = torch.zeros(scan_bytes, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.hpe_png_filter(table.ctypes.data_as(C.c_void_p), table_dev.data_ptr(), len(frames), buf.data_ptr(), buf.numel(), scan.data_ptr(),
                                      scan.numel(), st))
    for _ in range(2):
        scan.zero_()
        graph.replay()
        torch.cuda.synchronize()
        host = scan.cpu().numpy()
        for e, (n, _) in zip(table, CASES):
            w = want[n]
            assert np.array_equal(host[int(e["scan_offset"]):int(e["scan_offset"]) + w.size].reshape(w.shape), w), n


def test_pack_frames_in_its_three_input_forms():
    """batch_io.pack_frames on 1 x 1 x 3 (3 bytes), 4 x 4 x 1 (16 bytes exactly: no padding piece) and 3 x 5 x 3 (45 bytes) as a list, as
    [B,H,W,C] tensors and as decode_png_batch's DecodedBatch: the offsets, the buffer's bytes at them, and both encoders' channel clause"""
    frames = [E.content(h, w, c, seed=h + w) for h, w, c in ((1, 1, 3), (4, 4, 1), (3, 5, 3))]
    buf, shapes, offsets = batch_io.pack_frames([dev(f) for f in frames], png_encode.COLOR_TYPE)
    assert shapes == [(1, 1, 3), (4, 4, 1), (3, 5, 3)] and offsets == [0, 16, 32] and buf.numel() == 80
    host = buf.cpu().numpy()
    for f, o in zip(frames, offsets):
        assert np.array_equal(host[o:o + f.size], f.reshape(-1))
    assert not host[3:16].any() and not host[77:].any()  # the padding is zeros
    assert batch_io.pack_frames([dev(frames[1][:, :, 0])], [1])[1:] == ([(4, 4, 1)], [0])  # [H,W] is one channel

    for f in frames:  # a tensor is used as it lies: back to back, whatever the frame's size
        x = np.stack([f, f[::-1].copy()])
        buf, shapes, offsets = batch_io.pack_frames(dev(x), png_encode.COLOR_TYPE)
        assert shapes == [f.shape] * 2 and offsets == [0, f.size] and np.array_equal(buf.cpu().numpy(), x.reshape(-1))

    batch = hpe_amd.decode_png_batch([E.encode(f) for f in frames], channels=3)  # the grey frame comes back on three channels
    buf, shapes, offsets = batch_io.pack_frames(batch, png_encode.COLOR_TYPE)
    assert buf is batch.buffer and shapes == [(1, 1, 3), (4, 4, 3), (3, 5, 3)] and offsets == [0, 16, 64] and batch.nbytes == 112
    host = buf.cpu().numpy()
    for f, o in zip(frames, offsets):
        f3 = np.broadcast_to(f, f.shape[:2] + (3,))
        assert np.array_equal(host[o:o + f3.size], f3.reshape(-1))

    ok = dev(frames[0])
    for bad, channels, clause in ((4, jpeg_encode.CHANNELS, "1 or 3"), (2, jpeg_encode.CHANNELS, "1 or 3"), (2, png_encode.COLOR_TYPE, "1, 3 or 4")):
        with pytest.raises(hpe_amd.HpeError) as e:
            batch_io.pack_frames([ok, dev(np.zeros((2, 2, bad), np.uint8))], channels)
        assert str(e.value) == "image 1: %d channels: the channel count must be %s" % (bad, clause)
    assert batch_io.pack_frames([dev(np.zeros((2, 2, 4), np.uint8))], png_encode.COLOR_TYPE)[1] == [(2, 2, 4)]
    with pytest.raises(hpe_amd.HpeError, match=r"^image 0: 4 channels: the channel count must be 1 or 3$"):
        hpe_amd.encode_jpeg_batch(dev(np.zeros((1, 8, 8, 4), np.uint8)))
