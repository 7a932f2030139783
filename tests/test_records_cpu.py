"""hpe_amd.records without a GPU: CRC-32C, the TFRecord framing and its failures, the Example parser on a hand-encoded proto, and the
golden record files (tests/golden/records/, written by tests/golden/make_jpeg_golden.py through tests/records_writer.py)."""
import json
import os

import numpy as np
import pytest

import jpeg_ref as R
from hpe_amd import records, tf_checkpoint

RecordError = records.RecordError
crc32c = tf_checkpoint.crc32c

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "records")
IMAGES, MOCAP = os.path.join(GOLDEN, "images.tfrecords"), os.path.join(GOLDEN, "mocap.tfrecords")


def test_crc32c_check_value():
    assert crc32c(b"123456789") == 0xE3069283


def test_hand_encoded_example():
    """every byte written out: a packed float list, an unpacked float list, an int64 of -3, a bytes value, an unknown field and a
    repeated key"""
    def entry(key, feature):
        body = bytes([0x0A, len(key)]) + key + bytes([0x12, len(feature)]) + feature
        return bytes([0x0A, len(body)]) + body

    packed = bytes([0x12, 0x0A, 0x0A, 0x08, 0x00, 0x00, 0x80, 0x3F, 0x00, 0x00, 0x20, 0xC0])  # float_list { value: [1.0, -2.5] } packed
    unpacked = bytes([0x12, 0x0A, 0x0D, 0x00, 0x00, 0x00, 0x3F, 0x0D, 0x00, 0x00, 0x40, 0x40])  # float_list { value: 0.5 value: 3.0 }
    minus3 = bytes([0x1A, 0x0B, 0x08, 0xFD, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x01])  # int64_list { value: -3 }
    packed_ints = bytes([0x1A, 0x05, 0x0A, 0x03, 0x07, 0xAC, 0x02])  # int64_list { value: [7, 300] } packed
    raw = bytes([0x0A, 0x05, 0x0A, 0x03, 0x61, 0x00, 0xFF])  # bytes_list { value: "a\0\xff" }
    first = bytes([0x1A, 0x02, 0x08, 0x01])  # int64_list { value: 1 }, overwritten below
    features = entry(b"dup", first) + entry(b"p", packed) + entry(b"u", unpacked) + entry(b"n", minus3) + entry(b"pi", packed_ints) + \
        entry(b"b", raw) + bytes([0x78, 0x2A]) + entry(b"dup", minus3)  # 0x78: unknown field 15, varint 42
    payload = bytes([0x0A, len(features)]) + features + bytes([0x10, 0x07])  # plus an unknown field 2 of Example
    assert len(features) < 128
    f = records.parse_example(payload)
    assert sorted(f) == ["b", "dup", "n", "p", "pi", "u"]
    assert f["p"].dtype == np.float32 and f["p"].tolist() == [1.0, -2.5] and f["u"].tolist() == [0.5, 3.0]
    assert f["n"].dtype == np.int64 and f["n"].tolist() == [-3] and f["pi"].tolist() == [7, 300] and f["dup"].tolist() == [-3]
    assert f["b"] == [b"a\x00\xff"]
    with pytest.raises(RecordError):
        records.parse_example(payload[:-9])  # cut inside the last entry


def test_writer_and_reader_agree_on_unpacked_lists():
    import records_writer as RW

    p = RW.example([("f", RW.float_feature([1.5, -2.0], packed=False)), ("i", RW.int64_feature([-1, 2 ** 40], packed=False))])
    f = records.parse_example(p)
    assert f["f"].tolist() == [1.5, -2.0] and f["i"].tolist() == [-1, 2 ** 40]


def test_golden_image_records():
    want = json.load(open(os.path.join(GOLDEN, "images_expected.json")))
    got = [records.parse_image_example(p) for p in records.read_tfrecords(IMAGES)]
    assert len(got) == len(want) == 3 and len({(w["height"], w["width"]) for w in want}) == 3
    assert sum(w["face_pts"] is None for w in want) == 1
    for g, w in zip(got, want):
        assert g["image"] == R.stream(w["image"]) and g["seg"] == R.stream(w["seg"])
        assert (g["height"], g["width"], g["filename"]) == (w["height"], w["width"], w["filename"].encode())
        assert g["center"].tolist() == w["center"]
        kp = np.zeros((19, 3), np.float32)
        kp[:14, 0], kp[:14, 1], kp[:14, 2] = w["x"], w["y"], w["visibility"]
        if w["face_pts"] is not None:
            kp[14:] = np.array(w["face_pts"], np.float32).reshape(3, 5).T
        assert g["kp"].dtype == np.float32 and g["kp"].shape == (19, 3) and np.array_equal(g["kp"], kp)
        if w["face_pts"] is None:
            assert not g["kp"][14:].any()


def test_golden_mocap_records():
    rows = [records.parse_mocap_example(p) for p in records.read_tfrecords([MOCAP])]
    assert len(rows) == 4 and all(p.dtype == np.float32 and p.shape == (72,) and s.shape == (10,) for p, s in rows)
    assert np.array_equal(np.stack([p for p, _ in rows]), np.load(os.path.join(GOLDEN, "mocap_pose.npy")))
    assert np.array_equal(np.stack([s for _, s in rows]), np.load(os.path.join(GOLDEN, "mocap_shape.npy")))


def test_missing_key_and_wrong_length_name_the_key():
    import records_writer as RW

    with pytest.raises(RecordError, match="'shape'"):
        records.parse_mocap_example(RW.example([("pose", RW.float_feature([0.0] * 72))]))
    with pytest.raises(RecordError, match="'pose'"):
        records.parse_mocap_example(RW.mocap_example([0.0] * 71, [0.0] * 10))
    payload = next(records.read_tfrecords(IMAGES))
    feats = records.parse_example(payload)
    assert "image/center" in feats
    with pytest.raises(RecordError, match="'image/seg_gt'"):
        records.parse_image_example(RW.example([("image/encoded", RW.bytes_feature([b"x"])), ("image/x", RW.float_feature([0.0] * 14)),
                                                ("image/y", RW.float_feature([0.0] * 14)), ("image/visibility", RW.int64_feature([0] * 14))]))


def _damaged(tmp_path, name, edit):
    data = bytearray(open(IMAGES, "rb").read())
    data = edit(data)
    path = tmp_path / name
    path.write_bytes(bytes(data))
    return str(path)


def _second_record_offset():
    first = next(records.read_tfrecords(IMAGES))
    return 12 + len(first) + 4


def test_damage_raises_with_the_record_index(tmp_path):
    off = _second_record_offset()

    def flip(at):
        def edit(d):
            d[at] ^= 0x40
            return d
        return edit

    payload_flip = _damaged(tmp_path, "payload.tfrecords", flip(off + 12 + 100))
    with pytest.raises(RecordError, match=r"payload\.tfrecords: record 1: .*payload"):
        list(records.read_tfrecords(payload_flip))
    got = list(records.read_tfrecords(payload_flip, verify=False))  # the payload CRC alone is skipped
    assert len(got) == 3 and got[0] == next(records.read_tfrecords(IMAGES))
    with pytest.raises(RecordError, match="record 1: .*length"):
        list(records.read_tfrecords(_damaged(tmp_path, "length.tfrecords", flip(off + 1)), verify=False))
    with pytest.raises(RecordError, match="record 1: .*past the end"):
        list(records.read_tfrecords(_damaged(tmp_path, "cut_payload.tfrecords", lambda d: d[:off + 12 + 50])))
    with pytest.raises(RecordError, match="record 1: truncated header"):
        list(records.read_tfrecords(_damaged(tmp_path, "cut_header.tfrecords", lambda d: d[:off + 5])))
    assert len(list(records.read_tfrecords(_damaged(tmp_path, "whole.tfrecords", lambda d: d[:off])))) == 1


def test_record_dataset():
    ds = records.RecordDataset([IMAGES], batch_size=2)
    batches = list(ds)
    assert [len(b) for b in batches] == [2] and batches[0][1]["height"] == 40
    assert [len(b) for b in records.RecordDataset(IMAGES, 2, drop_last=False)] == [2, 1]
    ds = records.RecordDataset(MOCAP, 4, shuffle_seed=3, parse=records.parse_mocap_example)
    a, b = list(ds), list(ds)
    again = list(records.RecordDataset(MOCAP, 4, shuffle_seed=3, parse=records.parse_mocap_example))
    key = lambda batch: [float(p[0]) for p, _ in batch]  # noqa: E731
    assert key(a[0]) == key(again[0]) and sorted(key(a[0])) == sorted(key(b[0])) == sorted(np.load(os.path.join(GOLDEN, "mocap_pose.npy"))[:, 0].tolist())
