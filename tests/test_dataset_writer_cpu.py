"""The dataset writers without a GPU: the package's record writer reproduces the committed record files byte for byte (they were
written by tests/records_writer.py, which shares nothing with it but the CRC) and reads back through the reader; mat5_lite reads the
label fixtures scipy wrote and refuses what it does not read; the file pairing and the per-record rules of
src/util/create_dataset.py on a temporary tree.  LSP records need no mask re-encode, so a whole LSP file is written here."""
import json
import os
import types

import numpy as np
import pytest

import jpeg_ref as JR
from hpe_amd import datasets, mat5_lite, records

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REC, MAT, PNG = os.path.join(GOLDEN, "records"), os.path.join(GOLDEN, "mat5"), os.path.join(GOLDEN, "png")


def read(path):
    with open(path, "rb") as f:
        return f.read()


def expected_payloads():
    out = []
    for e in json.load(open(os.path.join(REC, "images_expected.json"))):
        out.append(records.image_example(JR.stream(e["image"]), JR.stream(e["seg"]), e["height"], e["width"], e["center"], e["filename"].encode(),
                                         e["x"], e["y"], e["visibility"], e["face_pts"]))
    return out


def test_writer_reproduces_the_image_records_byte_for_byte(tmp_path):
    path = tmp_path / "images.tfrecords"
    assert records.write_tfrecords(path, expected_payloads()) == 3
    assert read(path) == read(os.path.join(REC, "images.tfrecords"))


def test_writer_reproduces_the_mocap_records_byte_for_byte(tmp_path):
    pose, shape = np.load(os.path.join(REC, "mocap_pose.npy")), np.load(os.path.join(REC, "mocap_shape.npy"))
    path = tmp_path / "mocap.tfrecords"
    with records.TFRecordWriter(path) as w:
        for p, s in zip(pose, shape):
            w.write(records.mocap_example(p, s))
    assert w.count == len(pose) and read(path) == read(os.path.join(REC, "mocap.tfrecords"))


def test_what_is_written_reads_back(tmp_path):
    path = tmp_path / "x.tfrecords"
    records.write_tfrecords(path, expected_payloads())
    want = json.load(open(os.path.join(REC, "images_expected.json")))
    batches = list(records.RecordDataset(path, batch_size=3))
    assert len(batches) == 1
    for got, e in zip(batches[0], want):
        assert got["image"] == JR.stream(e["image"]) and got["seg"] == JR.stream(e["seg"]) and got["filename"] == e["filename"].encode()
        assert (got["height"], got["width"], got["center"].tolist()) == (e["height"], e["width"], e["center"])
        assert np.array_equal(got["kp"][:14, 0], np.array(e["x"], np.float32)) and np.array_equal(got["kp"][:14, 2], np.array(e["visibility"], np.float32))
        face = np.zeros(15, np.float32) if e["face_pts"] is None else np.array(e["face_pts"], np.float32)
        assert np.array_equal(got["kp"][14:].T.reshape(-1), face)


def test_serialize_example_types_and_negative_integers():
    payload = records.serialize_example({"b": [b"x", b""], "f": [1.5, -2.0], "i": [-1, 0, 1 << 40], "one": 7, "flag": np.array([True, False])})
    got = records.parse_example(payload)
    assert got["b"] == [b"x", b""] and got["f"].tolist() == [1.5, -2.0] and got["i"].tolist() == [-1, 0, 1 << 40] and got["one"].tolist() == [7]
    assert got["flag"].tolist() == [1, 0]
    with pytest.raises(records.RecordError, match="feature"):
        records.serialize_example({"bad": [object()]})


def test_mat5_lite_reads_the_fixtures():
    want = np.load(os.path.join(MAT, "expected.npz"))
    for name, keys in (("joints.mat", ["joints"]), ("joints_compressed.mat", ["joints", "count"]), ("small_types.mat", ["u8", "f32", "i16"])):
        got = mat5_lite.load(os.path.join(MAT, name))
        assert sorted(got) == sorted(keys)
        for k in keys:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k)


def test_mat5_lite_refuses_by_name(tmp_path):
    with pytest.raises(mat5_lite.MatError, match="variable 's' is a struct array"):
        mat5_lite.load(os.path.join(MAT, "struct.mat"))
    with pytest.raises(mat5_lite.MatError, match="variable 'c' is a cell array"):
        mat5_lite.load(os.path.join(MAT, "cell.mat"))
    whole = read(os.path.join(MAT, "joints.mat"))
    for cut in (60, 128 + 4, 128 + 8 + 40, len(whole) - 1):
        p = tmp_path / ("cut%d.mat" % cut)
        p.write_bytes(whole[:cut])
        with pytest.raises(mat5_lite.MatError, match="truncated"):
            mat5_lite.load(p)
    packed = read(os.path.join(MAT, "joints_compressed.mat"))
    p = tmp_path / "cutz.mat"
    p.write_bytes(packed[:len(packed) - 9])
    with pytest.raises(mat5_lite.MatError, match="truncated|inflate"):
        mat5_lite.load(p)
    p = tmp_path / "big.mat"
    p.write_bytes(whole[:126] + b"MI" + whole[128:])
    with pytest.raises(mat5_lite.MatError, match="big-endian"):
        mat5_lite.load(p)
    p = tmp_path / "v73.mat"
    p.write_bytes(b"MATLAB 7.3 MAT-file" + bytes(200))
    with pytest.raises(mat5_lite.MatError, match="v7.3"):
        mat5_lite.load(p)


def touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def test_filename_pairing_rules(tmp_path):
    base = lambda pairs: [(os.path.basename(a), os.path.basename(b)) for a, b in pairs]  # noqa: E731
    lsp_im, lsp_seg = str(tmp_path / "lsp" / "images"), str(tmp_path / "upi" / "lsp")
    for n in (3, 1, 2):
        touch(os.path.join(lsp_im, "im%04d.jpg" % n))
        touch(os.path.join(lsp_seg, "im%04d_segmentation.png" % n))
    touch(os.path.join(lsp_seg, "im00007_segmentation.png"))  # five digits: not LSP's pattern
    touch(os.path.join(lsp_seg, "im0001_part_segmentation.png"))
    assert base(datasets.filename_pairs_lsp(lsp_im, lsp_seg)) == [("im%04d.jpg" % n, "im%04d_segmentation.png" % n) for n in (1, 2, 3)]
    touch(os.path.join(lsp_im, "im0004.jpg"))
    with pytest.raises(ValueError, match="4 images but 3 segmentations"):
        datasets.filename_pairs_lsp(lsp_im, lsp_seg)
    e_im, e_seg = str(tmp_path / "lspet" / "images"), str(tmp_path / "upi-s1h" / "lsp_extended")
    for n in range(1, 7):
        touch(os.path.join(e_im, "im%05d.jpg" % n))
    for n in (5, 2):
        touch(os.path.join(e_seg, "im%05d_segmentation.png" % n))
    assert base(datasets.filename_pairs_lspe(e_im, e_seg)) == [("im00002.jpg", "im00002_segmentation.png"), ("im00005.jpg", "im00005_segmentation.png")]
    touch(os.path.join(e_seg, "im00009_segmentation.png"))
    with pytest.raises(ValueError, match="number 9, there are 6 images"):
        datasets.filename_pairs_lspe(e_im, e_seg)
    mpii = str(tmp_path / "mpii")
    for n in (12, 3):
        touch(os.path.join(mpii, "images", "%05d.png" % n))
        touch(os.path.join(mpii, "images", "%05d_segmentation.png" % n))
    touch(os.path.join(mpii, "images", "%05d_render.png" % 3))
    assert base(datasets.filename_pairs_mpii(mpii)) == [("00003.png", "00003_segmentation.png"), ("00012.png", "00012_segmentation.png")]


def test_record_fields_follow_the_reference_rules(tmp_path):
    img, seg = os.path.join(GOLDEN, "jpeg", "s420_37x43.jpg"), os.path.join(PNG, "rec_mask_37x43.png")
    label = np.zeros((3, 14))
    label[0], label[1] = np.linspace(3.0, 40.9, 14), np.linspace(30.5, 2.25, 14)
    label[2, [0, 13]] = 1
    keep = label.copy()
    f = datasets.record_fields(img, seg, label, "lsp_ext")  # the flag IS the visibility: joints 0 and 13
    assert np.array_equal(label, keep) and f["vis"].tolist() == [1] + [0] * 12 + [1]
    assert f["center"].tolist() == [int((3.0 + 40.9) / 2), int((30.5 + 2.25) / 2)] and f["center"].dtype == np.int64
    assert (f["height"], f["width"], f["filename"], f["face_pts"]) == (37, 43, "s420_37x43.jpg", None)
    assert f["image"] == read(img) and f["seg"] == read(seg)
    for ds in ("lsp", "mpii"):  # the flag is "occluded": every joint but 0 and 13 counts
        f = datasets.record_fields(img, seg, label, ds)
        assert f["vis"].tolist() == [0] + [1] * 12 + [0]
        assert f["center"].tolist() == [int((label[0, 1] + label[0, 12]) / 2), int((label[1, 1] + label[1, 12]) / 2)]
    wide = np.concatenate([label, np.arange(15, dtype=np.float64).reshape(3, 5)], axis=1)
    f = datasets.record_fields(seg, seg, wide, "lsp_ext")  # a PNG frame: IHDR gives the size
    assert f["face_pts"].tolist() == [float(v) for v in range(15)] and f["x"].shape == (14,) and (f["height"], f["width"]) == (37, 43)
    with pytest.raises(ValueError, match="no visible joint"):
        datasets.record_fields(img, seg, np.zeros((3, 14)), "lsp_ext")
    with pytest.raises(ValueError, match=r"\[3, 14\] or \[3, 19\]"):
        datasets.record_fields(img, seg, np.zeros((3, 16)), "lsp")


def test_labels_from_every_source_and_the_mpii_remap(tmp_path):
    want = np.load(os.path.join(MAT, "expected.npz"))["joints"]
    assert np.array_equal(datasets.load_labels(os.path.join(MAT, "joints.mat"), "lsp"), want)
    assert np.array_equal(datasets.load_labels(os.path.join(MAT, "joints_compressed.mat"), "lsp_ext"), want)
    assert np.array_equal(datasets.load_labels(want.transpose(1, 0, 2), "lsp_ext"), want)  # LSP-extended ships [14, 3, N]
    poses = np.random.RandomState(1).uniform(0, 100, (3, 16, 4))
    np.savez(tmp_path / "poses.npz", poses=poses)
    got = datasets.load_labels(tmp_path / "poses.npz", "mpii")
    assert got.shape == (3, 14, 4) and np.array_equal(got, poses[:, [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 8, 9], :])


def test_create_datasets_writes_the_lsp_files(tmp_path):
    """LSP keeps its PNG masks as they are, so both LSP files are written without a device; the split is at 1000 pairs"""
    lsp_dir, im, seg = tmp_path / "lsp", tmp_path / "lsp" / "images", tmp_path / "seg"
    os.makedirs(im)
    os.makedirs(seg)
    frame, mask = read(os.path.join(GOLDEN, "jpeg", "s422_rstrows_31x47.jpg")), read(os.path.join(PNG, "rec_mask_31x47.png"))
    for n in range(1, 1003):
        (im / ("im%04d.jpg" % n)).write_bytes(frame)
        (seg / ("im%04d_segmentation.png" % n)).write_bytes(mask)
    rng = np.random.RandomState(3)
    joints = rng.uniform(1, 30, (3, 14, 1002))
    joints[2] = rng.randint(0, 2, (14, 1002))
    joints[2, 0] = 0
    # a level-5 file written by hand: header, one miMATRIX of doubles
    body = (np.array([6, 8, 6, 0], "<u4").tobytes() + np.array([5, 12, 3, 14, 1002, 0], "<i4").tobytes() +
            np.array([1, 6], "<u4").tobytes() + b"joints\0\0" + np.array([9, joints.size * 8], "<u4").tobytes() + joints.astype("<f8").tobytes(order="F"))
    (lsp_dir / "joints.mat").write_bytes(b"MATLAB 5.0 MAT-file".ljust(124) + b"\x00\x01IM" + np.array([14, len(body)], "<u4").tobytes() + body)
    cfg = types.SimpleNamespace(dataset_dir=str(tmp_path / "out"), create_lsp=True, create_lsp_val=True, lsp_dir=str(lsp_dir), lsp_im=str(im) + os.sep,
                                lsp_seg=str(seg) + os.sep)
    wrote = datasets.create_datasets(cfg)
    assert {os.path.basename(k): v for k, v in wrote.items()} == {"lsp_train.tfrecords": 1000, "lsp_val.tfrecords": 2}
    val = [records.parse_image_example(p) for p in records.read_tfrecords(os.path.join(cfg.dataset_dir, "lsp_val.tfrecords"))]
    assert [v["filename"] for v in val] == [b"im1001.jpg", b"im1002.jpg"]
    for v, n in zip(val, (1001, 1002)):
        col = joints[:, :, n - 1]
        vis = col[2] == 0
        assert v["image"] == frame and v["seg"] == mask and (v["height"], v["width"]) == (31, 47)
        assert np.array_equal(v["kp"][:14, 0], col[0].astype(np.float32)) and np.array_equal(v["kp"][:14, 2], vis.astype(np.float32))
        assert v["center"].tolist() == ((col[:2, vis].min(axis=1) + col[:2, vis].max(axis=1)) / 2).astype(int).tolist()
    first = records.parse_image_example(next(records.read_tfrecords(os.path.join(cfg.dataset_dir, "lsp_train.tfrecords"))))
    assert first["filename"] == b"im0001.jpg"
