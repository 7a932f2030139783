"""GPU tests of the PNG decoder and of the mixed record path (run with -m gpu on an MI355X): ``decode_png_batch`` against the arrays the
fixtures were written from (tests/golden/make_png_golden.py), bit for bit -- PNG is lossless, the contract has no tolerance -- in one
batch of mixed sizes, colour types, depths and filters, alone, and in reverse order, with 3 channels and with 1; untouched padding and
guard bytes; determinism and graph replay of the two launches; ``decode_image_batch`` on interleaved JPEG and PNG streams against the
two decoders on the two subsets; ``load_training_batch`` on the golden records that mix PNG and JPEG against ``augment_batch`` on the
known pixels; and the refusal of a batch that holds one refused stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, jpeg, png, records

import jpeg_ref as JR
import png_ref as R
import png_writer as PW

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_png_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu
RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "records", "images_png.tfrecords")
NAMES = G.NAMES


@pytest.fixture(scope="module")
def streams():
    return [R.stream(n) for n in NAMES]


@pytest.fixture(scope="module")
def truths():
    return {(n, ch): G.truth(n, ch) for n in G.CASES for ch in (3, 1)}


def assert_truth(batch, names, channels, truths):
    assert len(batch) == len(names) and batch.buffer.dtype == torch.uint8 and batch.buffer.is_cuda
    host = batch.buffer.cpu().numpy()
    for name, (h, w), off in zip(names, batch.sizes.tolist(), batch.offsets.tolist()):
        want = truths[name, channels]
        assert off % 16 == 0 and (h, w) == want.shape[:2], name
        got = host[off:off + want.size].reshape(want.shape)
        diff = int((got != want).sum())
        assert diff == 0, "%s, %d channel(s): %d bytes differ, first at %s" % (name, channels, diff, np.argwhere(got != want)[0].tolist())


@pytest.mark.parametrize("channels", [3, 1])
def test_mixed_batch_equals_the_written_arrays(streams, truths, channels):
    assert_truth(hpe_amd.decode_png_batch(streams, channels=channels), NAMES, channels, truths)


@pytest.mark.parametrize("channels", [3, 1])
def test_reversed_batch_equals_the_written_arrays(streams, truths, channels):
    assert_truth(hpe_amd.decode_png_batch(streams[::-1], channels=channels, threads=3), NAMES[::-1], channels, truths)


@pytest.mark.parametrize("channels", [3, 1])
def test_single_image_batches_equal_the_written_arrays(streams, truths, channels):
    for name, s in zip(NAMES, streams):
        assert_truth(hpe_amd.decode_png_batch([s], channels=channels, threads=1), [name], channels, truths)


@pytest.mark.parametrize("channels", [3, 1])
def test_padding_and_guard_bytes_are_not_written(streams, truths, channels):
    _, table, totals = png.inflate_batch(streams, channels, threads=1)
    need = int(totals[2])
    out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    batch = hpe_amd.decode_png_batch(streams, channels=channels, out=out)
    assert batch.buffer.data_ptr() == out.data_ptr()
    assert_truth(batch, NAMES, channels, truths)
    host = out.cpu().numpy()
    written = np.zeros(need + 64, bool)
    for e in table:
        written[int(e["out_offset"]):int(e["out_offset"]) + int(e["H"]) * int(e["W"]) * channels] = True
    assert (~written).sum() >= 64 + 8 and (host[~written] == 0xA5).all()
    with pytest.raises(ValueError, match="need"):
        hpe_amd.decode_png_batch(streams, channels=channels, out=out[:need - 16])


def test_two_calls_give_the_same_bits(streams):
    a = hpe_amd.decode_png_batch(streams, channels=3)
    b = hpe_amd.decode_png_batch(streams, channels=3, threads=2)
    assert np.array_equal(a.offsets, b.offsets) and a.buffer.data_ptr() != b.buffer.data_ptr()
    for x, y in zip(a.frames, b.frames):
        assert torch.equal(x, y)


@pytest.mark.parametrize("channels", [3, 1])
def test_backend_launches_replay_from_a_graph(streams, truths, channels):
    """the launches of hpe_png_backend captured on one stream and replayed twice: the written arrays again, after the output was wiped"""
    staged, table, totals = png.inflate_batch(streams, channels, threads=4)
    raw_bytes, B = int(totals[0]), table.shape[0]
    staged_dev = torch.from_numpy(staged).cuda()
    workspace = torch.zeros(int(totals[1]), dtype=torch.uint8, device="cuda")
    out = torch.zeros(int(totals[2]), dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.hpe_png_backend(table.ctypes.data_as(C.c_void_p), staged_dev.data_ptr() + raw_bytes, B, staged_dev.data_ptr(), raw_bytes,
                                       workspace.data_ptr(), workspace.numel(), out.data_ptr(), out.numel(), st))
    batch = jpeg.DecodedBatch(out, np.stack([table["H"], table["W"]], axis=1).astype(np.int64), table["out_offset"].astype(np.int64), channels)
    for _ in range(2):
        out.zero_()
        workspace.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert_truth(batch, NAMES, channels, truths)


@pytest.mark.parametrize("channels", [3, 1])
def test_interleaved_jpeg_and_png_match_the_two_decoders(streams, channels):
    jnames = JR.CASES[:6]
    js = [JR.stream(n) for n in jnames]
    ps = streams[3:10]
    mixed, kind = [], []
    for i in range(max(len(js), len(ps))):  # P J P J ... and the longer list's tail
        for src, k in ((ps, "p"), (js, "j")):
            if i < len(src):
                mixed.append(src[i])
                kind.append((k, i))
    out = torch.full((1 << 17,), 0xA5, dtype=torch.uint8, device="cuda")
    got = hpe_amd.decode_image_batch(mixed, channels, threads=3, out=out)
    want = {"j": hpe_amd.decode_jpeg_batch(js, channels=channels).frames, "p": hpe_amd.decode_png_batch(ps, channels=channels).frames}
    assert len(got) == len(mixed) and got.buffer.data_ptr() == out.data_ptr()
    pos = 0
    written = torch.zeros_like(out, dtype=torch.bool)
    for frame, off, (k, i) in zip(got.frames, got.offsets.tolist(), kind):
        assert off == pos and torch.equal(frame, want[k][i]), (k, i)  # ONE packed buffer, in batch order
        written[off:off + frame.numel()] = True
        pos += (frame.numel() + 15) // 16 * 16
    assert bool((out[~written] == 0xA5).all())
    fresh = hpe_amd.decode_image_batch(mixed, channels)
    assert fresh.buffer.numel() == pos and all(torch.equal(a, b) for a, b in zip(fresh.frames, got.frames))
    only_p = hpe_amd.decode_image_batch(ps, channels)
    only_j = hpe_amd.decode_image_batch(js, channels)
    assert all(torch.equal(a, b) for a, b in zip(only_p.frames, want["p"])) and all(torch.equal(a, b) for a, b in zip(only_j.frames, want["j"]))


def test_load_training_batch_on_mixed_records_equals_augment_of_the_known_pixels(truths):
    """On the parent commit this fails: HpeError on the first PNG mask."""
    recs = [records.parse_image_example(p) for p in records.read_tfrecords(RECORDS)]
    frames = [JR.golden("s420_37x43", 3), JR.golden("s420_rstblocks_40x50", 3), truths["rec_frame_31x47", 3]]
    segs = [truths["rec_mask_37x43", 1], JR.golden("seg_40x50", 1), truths["rec_mask_31x47", 1]]
    assert [png.sniff(r["seg"]) for r in recs] == ["png", "jpeg", "png"] and [png.sniff(r["image"]) for r in recs] == ["jpeg", "jpeg", "png"]
    draws = {"trans": torch.tensor([[3, -7], [-12, 5], [0, 19]], dtype=torch.int32), "scale": torch.tensor([0.8, 1.0, 1.2229], dtype=torch.float32),
             "flip": torch.tensor([False, True, False])}
    got = hpe_amd.load_training_batch(recs, draws=draws)
    want = hpe_amd.augment_batch(frames, segs, np.stack([r["kp"] for r in recs]), np.stack([r["center"] for r in recs]), draws=draws)
    assert [tuple(t.shape) for t in got] == [(3, 224, 224, 3), (3, 224, 224), (3, 19, 3)]
    for g, w, what in zip(got, want, ("images", "seg_gts", "kp_gt")):
        assert g.dtype == torch.float32 and g.is_cuda and torch.equal(g.view(torch.int32), w.view(torch.int32)), what
    assert float(got[1].max()) > 0.5 and float(got[0].std()) > 0.05  # the comparison is not of blanks


def test_a_refused_stream_raises_before_anything_is_launched(streams):
    out = torch.full((1 << 17,), 0xA5, dtype=torch.uint8, device="cuda")
    c = G.case("rgb_3x5_idat7")
    laced = PW.write_png(c["samples"], 2, 8, 0, interlace=1)
    with pytest.raises(hpe_amd.HpeError, match="image 1: Adam7"):
        hpe_amd.decode_png_batch([streams[0], laced, streams[2]], channels=3, out=out)
    bad_row = PW.write_png(c["samples"], 2, 8, [0, 5, 0])
    with pytest.raises(hpe_amd.HpeError, match="image 2: row 1 has filter type 5"):
        hpe_amd.decode_png_batch([streams[0], streams[1], bad_row], channels=3, out=out)
    with pytest.raises(hpe_amd.HpeError, match="image 3: "):
        hpe_amd.decode_image_batch([streams[0], JR.stream(JR.CASES[0]), streams[1], JR.stream(JR.REFUSED[0])], 3, out=out)
    with pytest.raises(hpe_amd.HpeError, match="image 2: Adam7"):
        hpe_amd.decode_image_batch([JR.stream(JR.CASES[0]), streams[0], laced], 3, out=out)
    with pytest.raises(hpe_amd.HpeError, match="image 1: neither"):
        hpe_amd.decode_image_batch([streams[0], b"GIF89a" + bytes(20)], 3, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
