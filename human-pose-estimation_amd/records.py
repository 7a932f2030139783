"""The reference's training files without TensorFlow: ``*.tfrecords`` framing, ``tf.train.Example`` protos and the two parsers of
src/util/data_utils.py (``parse_example_proto`` :11-69, ``parse_mocap_example`` :109-127), plus ``load_training_batch``, the path from
parsed records to what ``GeneratorTrainer.step`` takes (src/data_loader.py:87-93, 160-213).  Everything but ``load_training_batch`` is
host code.  CRC-32C, varints and the protobuf wire format are those of tf_checkpoint.py.  The writers (``serialize_example``,
``image_example``, ``mocap_example``, ``write_tfrecords``, ``TFRecordWriter``) are the inverse: what ``tf.io.TFRecordWriter`` and
``tf.train.Example.SerializeToString`` produce, with packed lists and the features in the order given."""
from __future__ import annotations

import os
import struct

import numpy as np

from .tf_checkpoint import CheckpointError, _enc_varint, _pb_bytes, _proto_fields, _signed64, _varint, crc32c, mask_crc

NUM_KP = 19


class RecordError(ValueError):
    pass


def read_tfrecords(path_or_paths, verify=True):
    """Yield the payload of every record of one file or of several, in order.  Framing: uint64 length (LE), uint32 masked CRC-32C of
    the 8 length bytes, payload, uint32 masked CRC-32C of the payload.  A bad CRC, a truncated header or payload, or a length beyond
    the file raises RecordError with the file name and the record index.  verify=False skips the payload CRC only."""
    paths = [path_or_paths] if isinstance(path_or_paths, (str, bytes, os.PathLike)) else list(path_or_paths)
    for path in paths:
        name = os.fspath(path)
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            idx = 0
            while True:
                at = "%s: record %d: " % (name, idx)
                head = f.read(12)
                if not head:
                    break
                if len(head) < 12:
                    raise RecordError(at + "truncated header (%d of 12 bytes)" % len(head))
                length, len_crc = struct.unpack("<QI", head)
                if mask_crc(crc32c(head[:8])) != len_crc:
                    raise RecordError(at + "the CRC of the length does not match")
                if length + 4 > size - f.tell():
                    raise RecordError(at + "a payload of %d bytes runs past the end of the file (truncated?)" % length)
                body = f.read(length + 4)
                payload = body[:length]
                if verify and mask_crc(crc32c(payload)) != struct.unpack("<I", body[length:])[0]:
                    raise RecordError(at + "the CRC of the payload does not match")
                yield payload
                idx += 1


def _feature(buf):
    """one tf.train.Feature -> list[bytes] | float32 array | int64 array"""
    kind, out = None, []
    for fn, wt, v in _proto_fields(buf):
        if fn not in (1, 2, 3) or wt != 2:
            continue
        kind = fn
        for vfn, vwt, vv in _proto_fields(v):
            if vfn != 1:
                continue
            if fn == 1 and vwt == 2:
                out.append(vv)
            elif fn == 2 and vwt == 2:  # packed
                if len(vv) % 4:
                    raise RecordError("a packed float list of %d bytes" % len(vv))
                out.extend(np.frombuffer(vv, "<f4").tolist())
            elif fn == 2 and vwt == 5:
                out.append(struct.unpack("<f", struct.pack("<I", vv))[0])
            elif fn == 3 and vwt == 2:  # packed varints
                pos = 0
                while pos < len(vv):
                    x, pos = _varint(vv, pos)
                    out.append(_signed64(x & 0xFFFFFFFFFFFFFFFF))
            elif fn == 3 and vwt == 0:
                out.append(_signed64(vv & 0xFFFFFFFFFFFFFFFF))
            else:
                raise RecordError("a list value with wire type %d" % vwt)
    if kind == 2:
        return np.array(out, np.float32)
    if kind == 3:
        return np.array(out, np.int64)
    return out


def parse_example(payload):
    """A serialized tf.train.Example -> {name: float32 array | int64 array | list[bytes]}.  Example.features = 1, Features.feature = 1
    is the map (entry key 1, value 2); Feature: bytes_list = 1, float_list = 2, int64_list = 3, each list's value = 1, packed or not.
    Unknown fields are skipped; a key that appears twice takes the last value, as protobuf maps do."""
    out = {}
    try:
        for fn, wt, features in _proto_fields(payload):
            if fn != 1 or wt != 2:
                continue
            for efn, ewt, entry in _proto_fields(features):
                if efn != 1 or ewt != 2:
                    continue
                key, value = None, b""
                for kfn, kwt, kv in _proto_fields(entry):
                    if kfn == 1 and kwt == 2:
                        key = kv
                    elif kfn == 2 and kwt == 2:
                        value = kv
                if key is not None:
                    out[key.decode("utf-8")] = _feature(value)
    except RecordError:
        raise
    except (CheckpointError, UnicodeError, struct.error, OverflowError) as e:
        raise RecordError("corrupt Example: %s" % e) from e
    return out


def _need(feats, key, kind, count):
    if key not in feats:
        raise RecordError("the record lacks '%s'" % key)
    v = feats[key]
    ok = isinstance(v, list) if kind == "bytes" else isinstance(v, np.ndarray) and v.dtype == (np.float32 if kind == "float" else np.int64)
    if not ok or len(v) != count:
        raise RecordError("'%s' must hold %d %s value(s), got %d %s" % (key, count, kind, len(v), "bytes" if isinstance(v, list) else v.dtype))
    return v


def parse_image_example(payload):
    """``parse_example_proto`` without the decode: {'image', 'seg': JPEG or PNG bytes, 'height', 'width': int, 'center': int64 [2] (x, y),
    'filename': bytes, 'kp': float32 [19,3]}.  kp is the 14 image/x, image/y, image/visibility columns followed by image/face_pts
    reshaped [3,5] (all zeros when the record has none: the reference's default).  A missing key or a wrong length raises RecordError
    naming the key.  Where the record holds them: 'gt3d' float32 [14,3], 'pose' float32 [72], 'shape' float32 [10], 'has_3d' int."""
    f = parse_example(payload)
    label = np.zeros((3, NUM_KP), np.float32)
    label[0, :14] = _need(f, "image/x", "float", 14)
    label[1, :14] = _need(f, "image/y", "float", 14)
    label[2, :14] = _need(f, "image/visibility", "int64", 14).astype(np.float32)
    if "image/face_pts" in f:
        label[:, 14:] = _need(f, "image/face_pts", "float", 15).reshape(3, 5)
    out = {"image": _need(f, "image/encoded", "bytes", 1)[0], "seg": _need(f, "image/seg_gt", "bytes", 1)[0],
           "height": int(_need(f, "image/height", "int64", 1)[0]), "width": int(_need(f, "image/width", "int64", 1)[0]),
           "center": _need(f, "image/center", "int64", 2).copy(), "filename": _need(f, "image/filename", "bytes", 1)[0],
           "kp": np.ascontiguousarray(label.T)}
    # the optional 3-D ground truth: each key only where the record holds the feature
    if "mosh/gt3d" in f:
        out["gt3d"] = _need(f, "mosh/gt3d", "float", 42).reshape(14, 3).copy()
    if "mosh/pose" in f:
        out["pose"] = _need(f, "mosh/pose", "float", 72).copy()
    if "mosh/shape" in f:
        out["shape"] = _need(f, "mosh/shape", "float", 10).copy()
    if "meta/has_3d" in f:
        out["has_3d"] = int(_need(f, "meta/has_3d", "int64", 1)[0])
    return out


def parse_mocap_example(payload):
    """-> (pose float32 [72], shape float32 [10])"""
    f = parse_example(payload)
    return _need(f, "pose", "float", 72).copy(), _need(f, "shape", "float", 10).copy()


class RecordDataset:
    """Batches of parsed records from one or several files: iterating yields lists of ``batch_size`` values of ``parse`` (default
    ``parse_image_example``).  With ``shuffle_seed`` the records are read once and every pass walks a new permutation, drawn from
    RandomState(shuffle_seed + pass); without it the files are streamed in order.  Host-only: nothing is decoded here.

    shard=(rank, world): data-parallel training.  ``batch_size`` stays the GLOBAL batch: every rank walks the same global batches (the
    same files, the same ``shuffle_seed``) and yields only its ``distributed.shard_bounds`` slice of each, cut before ``parse`` so that
    only that slice is parsed; the ranks' batches, concatenated in rank order, are the single-process batch.  shard_unit: rows that
    stay together (the mocap rows of one image: ``num_stage``); the bounds are taken over batch / shard_unit units."""

    def __init__(self, paths, batch_size, shuffle_seed=None, drop_last=True, parse=parse_image_example, verify=True, shard=None, shard_unit=1):
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        if shard is not None:
            rank, world = (int(v) for v in shard)
            if world < 1 or not 0 <= rank < world:
                raise ValueError("shard must be (rank, world) with 0 <= rank < world")
            if int(shard_unit) < 1 or int(batch_size) % int(shard_unit):
                raise ValueError("shard_unit must divide batch_size")
            shard = (rank, world)
        self.shard, self.shard_unit = shard, int(shard_unit)
        self.paths = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
        self.batch_size, self.shuffle_seed, self.drop_last, self.parse, self.verify = int(batch_size), shuffle_seed, bool(drop_last), parse, verify
        self._payloads, self._pass = None, 0

    def _ordered(self):
        if self.shuffle_seed is None:
            return read_tfrecords(self.paths, self.verify)
        if self._payloads is None:
            self._payloads = list(read_tfrecords(self.paths, self.verify))
        order = np.random.RandomState(int(self.shuffle_seed) + self._pass).permutation(len(self._payloads))
        self._pass += 1
        return (self._payloads[i] for i in order)

    def _mine(self, payloads):
        """this rank's slice of one global batch (a short last batch is cut over the units it has)"""
        from .distributed import shard_bounds

        u = self.shard_unit
        lo, hi = shard_bounds(len(payloads) // u, *self.shard)
        return payloads[lo * u:hi * u]

    def __iter__(self):
        if self.shard is None:
            batch = []
            for payload in self._ordered():
                batch.append(self.parse(payload))
                if len(batch) == self.batch_size:
                    yield batch
                    batch = []
            if batch and not self.drop_last:
                yield batch
            return
        batch = []
        for payload in self._ordered():
            batch.append(payload)
            if len(batch) == self.batch_size:
                yield [self.parse(p) for p in self._mine(batch)]
                batch = []
        if batch and not self.drop_last:
            yield [self.parse(p) for p in self._mine(batch)]


def _feature_bytes(value):
    """one value -> a serialized tf.train.Feature: bytes or a list of bytes -> bytes_list; a float array, a float or a list holding a
    float -> float_list (float32, packed); integers and bools -> int64_list (packed varints, a negative value as 10 bytes)"""
    if isinstance(value, (bytes, bytearray, memoryview)):
        value = [bytes(value)]
    if isinstance(value, (list, tuple)) and value and all(isinstance(v, (bytes, bytearray, memoryview)) for v in value):
        return _pb_bytes(1, b"".join(_pb_bytes(1, bytes(v)) for v in value))
    arr = np.asarray(value)
    if arr.dtype.kind == "f":
        return _pb_bytes(2, _pb_bytes(1, arr.astype("<f4").reshape(-1).tobytes()))
    if arr.dtype.kind in "iub":
        return _pb_bytes(3, _pb_bytes(1, b"".join(_enc_varint(int(v) & 0xFFFFFFFFFFFFFFFF) for v in arr.reshape(-1).tolist())))
    raise RecordError("a feature must be bytes, a list of bytes, floats or integers, not %s" % (arr.dtype if arr.dtype != object else type(value).__name__))


def serialize_example(features):
    """A tf.train.Example of ``features`` -- a dict, or a list of (name, value) pairs, kept in order -> bytes.  The value decides the
    list type (``_feature_bytes``).  ``parse_example`` is the inverse."""
    items = features.items() if isinstance(features, dict) else features
    entries = b"".join(_pb_bytes(1, _pb_bytes(1, str(k).encode("utf-8")) + _pb_bytes(2, _feature_bytes(v))) for k, v in items)
    return _pb_bytes(1, entries)


def image_example(image, seg, height, width, center, filename, x, y, vis, face_pts=None, gt3d=None, pose=None, shape=None):
    """The record of src/util/create_dataset.py:52-70: image and mask bytes as they are, height, width, the file's base name, format
    b"JPEG", center int64 [2] (x, y), the 14 visibilities (int64) and coordinates (float), and the 15 face floats if there are any.
    Optional 3-D ground truth (DESIGN.md "3-D pose scores"): gt3d [14,3] joints in metres -> mosh/gt3d (42 floats), pose [72] ->
    mosh/pose, shape [10] -> mosh/shape, and meta/has_3d = 1 when any of them is given; without them the bytes are what they always were."""
    name = filename if isinstance(filename, (bytes, bytearray)) else str(filename).encode("utf-8")
    feats = [("image/encoded", bytes(image)), ("image/seg_gt", bytes(seg)), ("image/height", [int(height)]), ("image/width", [int(width)]),
             ("image/filename", bytes(name)), ("image/format", b"JPEG"), ("image/center", np.asarray(center, np.int64)),
             ("image/visibility", np.asarray(vis, np.int64)), ("image/x", np.asarray(x, np.float32)), ("image/y", np.asarray(y, np.float32))]
    if face_pts is not None:
        feats.append(("image/face_pts", np.asarray(face_pts, np.float32)))
    extra = [(key, np.asarray(v, np.float32).reshape(-1), n) for key, v, n in (("mosh/gt3d", gt3d, 42), ("mosh/pose", pose, 72), ("mosh/shape", shape, 10))
             if v is not None]
    for key, v, n in extra:
        if v.size != n:
            raise RecordError("'%s' must hold %d floats, got %d" % (key, n, v.size))
        feats.append((key, v))
    if extra:
        feats.append(("meta/has_3d", [1]))
    return serialize_example(feats)


def mocap_example(pose, shape):
    return serialize_example([("pose", np.asarray(pose, np.float32)), ("shape", np.asarray(shape, np.float32))])


def frame_record(payload):
    """one record's bytes: uint64 length, its masked CRC-32C, the payload, its masked CRC-32C"""
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", mask_crc(crc32c(head))) + bytes(payload) + struct.pack("<I", mask_crc(crc32c(payload)))


class TFRecordWriter:
    """``with TFRecordWriter(path) as w: w.write(payload)`` -- a ``*.tfrecords`` file ``read_tfrecords`` and TensorFlow read"""

    def __init__(self, path):
        self._f = open(path, "wb")
        self.count = 0

    def write(self, payload):
        self._f.write(frame_record(payload))
        self.count += 1

    def close(self):
        if not self._f.closed:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_tfrecords(path, payloads):
    """every payload as one record of ``path`` -> the number written"""
    with TFRecordWriter(path) as w:
        for p in payloads:
            w.write(p)
        return w.count


def load_training_batch(records, draws=None, generator=None, threads=None, **augment_args):
    """Parsed image records (``parse_image_example`` dicts, or serialized payloads) -> the (images [B,224,224,3], seg_gts [B,224,224],
    kp_gt [B,19,3]) CUDA triple that ``GeneratorTrainer.step`` takes: ``image`` decoded with 3 channels and ``seg`` with 1, one
    ``decode_image_batch`` each (every stream a JPEG or a PNG, side by side in one batch), then ``augment_batch`` on the decoded buffers as they are.  draws / generator / further keyword
    arguments are ``augment_batch``'s.  A record whose streams do not have its height and width raises RecordError."""
    from .augment import augment_batch
    from .batch_io import DEFAULT_THREADS
    from .png import decode_image_batch

    recs = [parse_image_example(r) if isinstance(r, (bytes, bytearray, memoryview)) else r for r in records]
    if not recs:
        raise ValueError("records is empty")
    threads = DEFAULT_THREADS if threads is None else threads
    frames = decode_image_batch([r["image"] for r in recs], channels=3, threads=threads)
    segs = decode_image_batch([r["seg"] for r in recs], channels=1, threads=threads)
    for i, r in enumerate(recs):
        for what, d in (("image/encoded", frames), ("image/seg_gt", segs)):
            if tuple(d.sizes[i]) != (r["height"], r["width"]):
                raise RecordError("record %d: '%s' decodes to %s, the record says %s" % (i, what, d.sizes[i].tolist(), [r["height"], r["width"]]))
    kp = np.stack([r["kp"] for r in recs]).astype(np.float32)
    centers = np.stack([np.asarray(r["center"]) for r in recs]).astype(np.int32)
    return augment_batch(frames, segs, kp, centers, draws=draws, generator=generator, **augment_args)


def load_training_batch_3d(records, engine, draws=None, generator=None, threads=None, **augment_args):
    """``load_training_batch`` with the records' 3-D ground truth: -> (images, seg_gts, kp_gt, gt), gt the ``ops.Gt3D`` of
    ``augment.gt3d_real(engine, records, draws["flip"])``.  The draws are made HERE when ``draws`` is None, with the generator and the
    ``trans_max`` / ``scale_range`` that ``augment_batch`` would use, so the first three outputs are bit-identical to
    ``load_training_batch`` from the same generator state and the generator is left as it would be; the labels in ``gt`` stay
    unflipped, the flip draw travels with them and the loss mirrors them."""
    from .augment import SCALE_RANGE, TRANS_MAX, draw_augmentation, gt3d_real

    recs = [parse_image_example(r) if isinstance(r, (bytes, bytearray, memoryview)) else r for r in records]
    if not recs:
        raise ValueError("records is empty")
    if draws is None:
        draws = draw_augmentation(len(recs), generator=generator, trans_max=augment_args.get("trans_max", TRANS_MAX),
                                  scale_range=augment_args.get("scale_range", SCALE_RANGE))
    images, seg_gts, kp_gt = load_training_batch(recs, draws=draws, threads=threads, **augment_args)
    return images, seg_gts, kp_gt, gt3d_real(engine, recs, draws["flip"])
