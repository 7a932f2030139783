"""GPU test of the dataset writers (run with -m gpu on an MI355X): an LSP-extended-style tree built from the committed JPEG frames and
PNG masks becomes a record file whose ``image/seg_gt`` is, byte for byte, what Pillow's libjpeg-turbo encodes of the mask's channel 0
(tests/golden/make_jpeg_encode_golden.py), and ``load_training_batch`` of that file equals ``augment_batch`` on the known pixels."""
import os
import shutil

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import datasets, records

import jpeg_encode_ref as R
import jpeg_ref as JR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# image number -> (frame fixture, mask fixture); number 2 has no mask, as most LSP-extended frames
TREE = {1: ("s420_37x43", "rec_mask_37x43"), 2: ("s420_5x4", None), 3: ("s422_rstrows_31x47", "rec_mask_31x47")}


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    root = tmp_path_factory.mktemp("lspet")
    im, seg = root / "images", root / "upi" / "lsp_extended"
    os.makedirs(im)
    os.makedirs(seg)
    for n, (frame, mask) in TREE.items():
        shutil.copy(os.path.join(GOLDEN, "jpeg", frame + ".jpg"), im / ("im%05d.jpg" % n))
        if mask:
            shutil.copy(os.path.join(GOLDEN, "png", mask + ".png"), seg / ("im%05d_segmentation.png" % n))
    rng = np.random.RandomState(11)
    labels = np.zeros((14, 3, 3))  # LSP-extended's own axis order
    labels[:, 0], labels[:, 1], labels[:, 2] = rng.uniform(2, 30, (14, 3)), rng.uniform(2, 30, (14, 3)), rng.randint(0, 2, (14, 3))
    labels[0, 2] = 1
    pairs = datasets.filename_pairs_lspe(str(im), str(seg))
    path = root / "lsp_ext.tfrecords"
    count = datasets.create_records(path, pairs, labels, "lsp_ext", batch=2)
    return path, count, labels, pairs


def test_seg_gt_is_pillows_encode_of_channel_zero(written):
    path, count, labels, pairs = written
    assert count == 2 and [os.path.basename(a) for a, _ in pairs] == ["im00001.jpg", "im00003.jpg"]
    recs = [records.parse_image_example(p) for p in records.read_tfrecords(path)]
    for r, n in zip(recs, (1, 3)):
        frame, mask = TREE[n]
        assert r["seg"] == R.stream("seg_" + mask), "image/seg_gt of %s: %d bytes, Pillow wrote %d" % (mask, len(r["seg"]), len(R.stream("seg_" + mask)))
        assert r["image"] == JR.stream(frame) and r["filename"] == ("im%05d.jpg" % n).encode()
        assert (r["height"], r["width"]) == JR.golden(frame, 3).shape[:2]
        col = labels[:, :, n - 1].T
        vis = col[2].astype(bool)
        assert np.array_equal(r["kp"][:14, 2], vis.astype(np.float32)) and np.array_equal(r["kp"][:14, 0], col[0].astype(np.float32))
        assert r["center"].tolist() == ((col[:2, vis].min(axis=1) + col[:2, vis].max(axis=1)) / 2).astype(int).tolist()
    one = datasets.image_record(pairs[1][0], pairs[1][1], labels[:, :, 2].T, "lsp_ext")  # the single-record path writes the same bytes
    assert one == list(records.read_tfrecords(path))[1]


def test_load_training_batch_of_the_written_file_equals_augment_of_the_known_pixels(written):
    path = written[0]
    recs = [records.parse_image_example(p) for p in records.read_tfrecords(path)]
    frames = [JR.golden(TREE[n][0], 3) for n in (1, 3)]
    segs = [R.decoded("seg_" + TREE[n][1]) for n in (1, 3)]
    draws = {"trans": torch.tensor([[3, -7], [-12, 5]], dtype=torch.int32), "scale": torch.tensor([0.8, 1.2229], dtype=torch.float32),
             "flip": torch.tensor([False, True])}
    got = hpe_amd.load_training_batch(recs, draws=draws)
    want = hpe_amd.augment_batch(frames, segs, np.stack([r["kp"] for r in recs]), np.stack([r["center"] for r in recs]), draws=draws)
    assert [tuple(t.shape) for t in got] == [(2, 224, 224, 3), (2, 224, 224), (2, 19, 3)]
    for g, w, what in zip(got, want, ("images", "seg_gts", "kp_gt")):
        assert g.dtype == torch.float32 and g.is_cuda and torch.equal(g.view(torch.int32), w.view(torch.int32)), what
    assert float(got[1].max()) > 0.5 and float(got[0].std()) > 0.05  # the comparison is not of blanks
