"""GPU tests of the JPEG decoder and the record path (run with -m gpu on an MI355X): ``decode_jpeg_batch`` against the pixels
libjpeg-turbo decoded when the fixtures were made (tests/golden/jpeg/), bit for bit -- the contract has no tolerance -- in one batch of
mixed sizes and samplings, alone, and in reverse order; untouched padding and guard bytes; determinism and graph replay of the two
back-end launches; ``load_training_batch`` on the golden records against ``augment_batch`` on the golden pixels; and the refusal of a
batch that holds one stream outside the subset."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import _lib, jpeg, records

import jpeg_ref as R

pytestmark = pytest.mark.gpu
RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "records", "images.tfrecords")


@pytest.fixture(scope="module")
def streams():
    return [R.stream(n) for n in R.CASES]


def assert_golden(batch, names, channels):
    assert len(batch) == len(names) and batch.buffer.dtype == torch.uint8 and batch.buffer.is_cuda
    for name, frame, (h, w), off in zip(names, batch.frames, batch.sizes.tolist(), batch.offsets.tolist()):
        want = R.golden(name, channels)
        assert off % 16 == 0 and tuple(frame.shape) == want.shape and (h, w) == want.shape[:2], name
        diff = int((frame.cpu().numpy() != want).sum())
        assert diff == 0, "%s, %d channel(s): %d bytes differ" % (name, channels, diff)


@pytest.mark.parametrize("channels", [3, 1])
def test_mixed_batch_equals_golden(streams, channels):
    assert_golden(hpe_amd.decode_jpeg_batch(streams, channels=channels), R.CASES, channels)


@pytest.mark.parametrize("channels", [3, 1])
def test_reversed_batch_equals_golden(streams, channels):
    assert_golden(hpe_amd.decode_jpeg_batch(streams[::-1], channels=channels, threads=3), R.CASES[::-1], channels)


@pytest.mark.parametrize("channels", [3, 1])
def test_single_image_batches_equal_golden(streams, channels):
    for name, s in zip(R.CASES, streams):
        assert_golden(hpe_amd.decode_jpeg_batch([s], channels=channels, threads=1), [name], channels)


@pytest.mark.parametrize("channels", [3, 1])
def test_padding_and_guard_bytes_are_not_written(streams, channels):
    _, table, totals = jpeg.entropy_decode(streams, channels, threads=1)
    need = int(totals[2])
    out = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    batch = hpe_amd.decode_jpeg_batch(streams, channels=channels, out=out)
    assert batch.buffer.data_ptr() == out.data_ptr()
    assert_golden(batch, R.CASES, channels)
    host = out.cpu().numpy()
    written = np.zeros(need + 64, bool)
    for e in table:
        written[int(e["out_offset"]):int(e["out_offset"]) + int(e["H"]) * int(e["W"]) * channels] = True
    assert (~written).sum() >= 64 + 8 and (host[~written] == 0xA5).all()
    with pytest.raises(ValueError, match="need"):
        hpe_amd.decode_jpeg_batch(streams, channels=channels, out=out[:need - 16])


def test_two_calls_give_the_same_bits(streams):
    a = hpe_amd.decode_jpeg_batch(streams, channels=3)
    b = hpe_amd.decode_jpeg_batch(streams, channels=3, threads=2)
    assert np.array_equal(a.offsets, b.offsets) and a.buffer.data_ptr() != b.buffer.data_ptr()
    for x, y in zip(a.frames, b.frames):
        assert torch.equal(x, y)


def test_backend_launches_replay_from_a_graph(streams):
    """the two launches of hpe_jpeg_backend captured on one stream and replayed twice: the goldens again, after the output was wiped"""
    coef, table, totals = jpeg.entropy_decode(streams, 3, threads=4)
    n, B = coef.shape[0], table.shape[0]
    coef_dev = torch.from_numpy(coef).cuda()
    table_dev = torch.from_numpy(table.view(np.uint8).copy()).cuda()
    workspace = torch.zeros(int(totals[1]), dtype=torch.uint8, device="cuda")
    out = torch.zeros(int(totals[2]), dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.hpe_jpeg_backend(table.ctypes.data_as(C.c_void_p), table_dev.data_ptr(), B, coef_dev.data_ptr(), n, workspace.data_ptr(),
                                        workspace.numel(), out.data_ptr(), out.numel(), st))
    batch = jpeg.DecodedBatch(out, np.stack([table["H"], table["W"]], axis=1).astype(np.int64), table["out_offset"].astype(np.int64), 3)
    for _ in range(2):
        out.zero_()
        workspace.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert_golden(batch, R.CASES, 3)


def test_load_training_batch_equals_augment_of_the_golden_pixels():
    recs = [records.parse_image_example(p) for p in records.read_tfrecords(RECORDS)]
    names = ("s420_37x43", "s420_rstblocks_40x50", "s422_rstrows_31x47")
    segs = ("seg_37x43", "seg_40x50", "seg_31x47")
    draws = {"trans": torch.tensor([[3, -7], [-12, 5], [0, 19]], dtype=torch.int32), "scale": torch.tensor([0.8, 1.0, 1.2229], dtype=torch.float32),
             "flip": torch.tensor([False, True, False])}
    got = hpe_amd.load_training_batch(recs, draws=draws)
    want = hpe_amd.augment_batch([R.golden(n, 3) for n in names], [R.golden(n, 1) for n in segs], np.stack([r["kp"] for r in recs]),
                                 np.stack([r["center"] for r in recs]), draws=draws)
    assert [tuple(t.shape) for t in got] == [(3, 224, 224, 3), (3, 224, 224), (3, 19, 3)]
    for g, w, what in zip(got, want, ("images", "seg_gts", "kp_gt")):
        assert g.dtype == torch.float32 and g.is_cuda and torch.equal(g.view(torch.int32), w.view(torch.int32)), what
    assert float(got[1].max()) > 0.5 and float(got[0].std()) > 0.05  # the comparison is not of blanks
    again = hpe_amd.load_training_batch(list(records.read_tfrecords(RECORDS)), draws=draws)  # serialized payloads are parsed here
    assert all(torch.equal(a, g) for a, g in zip(again, got))


def test_a_refused_stream_raises_before_anything_is_launched(streams):
    out = torch.full((1 << 16,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(hpe_amd.HpeError, match="image 1: progressive"):
        hpe_amd.decode_jpeg_batch([streams[0], R.stream(R.REFUSED[0]), streams[2]], channels=3, out=out)
    with pytest.raises(hpe_amd.HpeError, match="image 2: "):
        hpe_amd.decode_jpeg_batch([streams[0], streams[1], streams[2][:-40]], channels=3, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
