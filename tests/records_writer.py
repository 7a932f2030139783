"""Writer of ``*.tfrecords`` files of ``tf.train.Example`` protos for the tests: the inverse of hpe_amd.records, written from the
format's definition and sharing nothing with the reader but the CRC."""
import struct

from hpe_amd import tf_checkpoint

crc32c, mask_crc = tf_checkpoint.crc32c, tf_checkpoint.mask_crc


def varint(v):
    v &= 0xFFFFFFFFFFFFFFFF  # a negative int64 is its 10-byte two's complement
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        out.append(b | (0x80 if v else 0))
        if not v:
            return bytes(out)


def field(number, payload):
    """a length-delimited field"""
    return varint(number << 3 | 2) + varint(len(payload)) + payload


def bytes_feature(values):
    return field(1, b"".join(field(1, v) for v in values))


def float_feature(values, packed=True):
    if packed:
        return field(2, field(1, struct.pack("<%df" % len(values), *values)))
    return field(2, b"".join(varint(1 << 3 | 5) + struct.pack("<f", v) for v in values))


def int64_feature(values, packed=True):
    if packed:
        return field(3, field(1, b"".join(varint(int(v)) for v in values)))
    return field(3, b"".join(varint(1 << 3 | 0) + varint(int(v)) for v in values))


def example(features):
    """features: a list of (name, serialized Feature) pairs, kept in order (a name may repeat)"""
    entries = b"".join(field(1, field(1, k.encode()) + field(2, v)) for k, v in features)
    return field(1, entries)


def record(payload):
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", mask_crc(crc32c(head))) + payload + struct.pack("<I", mask_crc(crc32c(payload)))


def write_tfrecords(path, payloads):
    with open(path, "wb") as f:
        for p in payloads:
            f.write(record(p))


def image_example(image, seg, height, width, center, filename, x, y, vis, face_pts=None):
    feats = [("image/encoded", bytes_feature([image])), ("image/seg_gt", bytes_feature([seg])), ("image/height", int64_feature([height])),
             ("image/width", int64_feature([width])), ("image/filename", bytes_feature([filename])), ("image/format", bytes_feature([b"JPEG"])),
             ("image/center", int64_feature(center)), ("image/visibility", int64_feature(vis)), ("image/x", float_feature(x)),
             ("image/y", float_feature(y))]
    if face_pts is not None:
        feats.append(("image/face_pts", float_feature(face_pts)))
    return example(feats)


def mocap_example(pose, shape):
    return example([("pose", float_feature(pose)), ("shape", float_feature(shape))])
