"""TensorBoard event files without TensorFlow: what the reference's ``tf.summary.create_file_writer`` / ``tf.summary.scalar`` /
``tf.summary.image`` leave on disk (src/trainer.py:96-103, 747-809), written and read back here.  A file is TFRecord framing (records.py:
length, masked CRC-32C of the length, payload, masked CRC-32C of the payload) around ``Event`` protos: the first is
``Event{wall_time, file_version "brain.Event:2"}``, then one ``Event{wall_time, step, summary{value{tag, simple_value | image}}}`` per
call.  Field numbers: Event 1 wall_time (double), 2 step (int64), 3 file_version (string), 5 summary; Summary 1 value; Value 1 tag,
2 simple_value (float, fixed32), 4 image; Image 1 height, 2 width, 3 colorspace, 4 encoded_image_string.  Fields are written in ascending
order; a zero ``wall_time`` or ``step`` is omitted as proto3 omits defaults, while ``simple_value`` and ``image`` are members of the
Value's oneof and are written whenever set, 0.0 included.  Host code; only ``image`` with a frame reaches the device (encode_png_batch).
PARITY UNPINNED: no TensorBoard is installed where this was written (DESIGN.md "Training summaries")."""
from __future__ import annotations

import os
import socket
import struct
import time

from .records import RecordError, read_tfrecords
from .tf_checkpoint import _enc_varint, _pb_bytes, _pb_fixed32, _pb_varint, _proto_fields, _signed64, crc32c, mask_crc

FILE_VERSION = "brain.Event:2"


def _pb_double(fn, v):
    return _enc_varint((fn << 3) | 1) + struct.pack("<d", v)


def encode_event(wall_time, step=0, values=(), file_version=None):
    """One Event proto.  values: (tag, float) or (tag, {"height", "width", "colorspace", "encoded_image_string"}) pairs."""
    out = b""
    if wall_time != 0.0:
        out += _pb_double(1, float(wall_time))
    if step != 0:
        out += _pb_varint(2, int(step) & 0xFFFFFFFFFFFFFFFF)
    if file_version is not None:
        out += _pb_bytes(3, file_version.encode("utf-8"))
    if values:
        summary = b""
        for tag, v in values:
            body = _pb_bytes(1, tag.encode("utf-8")) if tag else b""
            if isinstance(v, dict):
                img = b"".join(_pb_varint(fn, int(v[k])) for fn, k in ((1, "height"), (2, "width"), (3, "colorspace")) if int(v[k]) != 0)
                if v["encoded_image_string"]:
                    img += _pb_bytes(4, bytes(v["encoded_image_string"]))
                body += _pb_bytes(4, img)
            else:
                body += _pb_fixed32(2, struct.unpack("<I", struct.pack("<f", float(v)))[0])
            summary += _pb_bytes(1, body)
        out += _pb_bytes(5, summary)
    return out


def frame_record(payload):
    """TFRecord framing of one payload"""
    head = struct.pack("<Q", len(payload))
    return head + struct.pack("<I", mask_crc(crc32c(head))) + payload + struct.pack("<I", mask_crc(crc32c(payload)))


def decode_event(payload):
    """-> {"wall_time", "step", "values": [{"tag", "simple_value"} | {"tag", "image": {...}}]} (+ "file_version" when present)"""
    ev = {"wall_time": 0.0, "step": 0, "values": []}
    for fn, wt, v in _proto_fields(payload):
        if fn == 1 and wt == 1:
            ev["wall_time"] = struct.unpack("<d", int(v).to_bytes(8, "little"))[0]
        elif fn == 2 and wt == 0:
            ev["step"] = _signed64(v & 0xFFFFFFFFFFFFFFFF)
        elif fn == 3 and wt == 2:
            ev["file_version"] = bytes(v).decode("utf-8")
        elif fn == 5 and wt == 2:
            for sfn, swt, sv in _proto_fields(v):
                if sfn != 1 or swt != 2:
                    continue
                val = {"tag": ""}
                for vfn, vwt, vv in _proto_fields(sv):
                    if vfn == 1 and vwt == 2:
                        val["tag"] = bytes(vv).decode("utf-8")
                    elif vfn == 2 and vwt == 5:
                        val["simple_value"] = struct.unpack("<f", int(vv).to_bytes(4, "little"))[0]
                    elif vfn == 4 and vwt == 2:
                        img = {"height": 0, "width": 0, "colorspace": 0, "encoded_image_string": b""}
                        for ifn, iwt, iv in _proto_fields(vv):
                            if ifn in (1, 2, 3) and iwt == 0:
                                img[("height", "width", "colorspace")[ifn - 1]] = int(iv)
                            elif ifn == 4 and iwt == 2:
                                img["encoded_image_string"] = bytes(iv)
                        val["image"] = img
                ev["values"].append(val)
    return ev


def read_events(path, verify=True):
    """Every event of one file (or of several), in order, as ``decode_event`` returns them.  A bad CRC or a truncated record raises
    RecordError, as ``read_tfrecords`` does."""
    return [decode_event(p) for p in read_tfrecords(path, verify)]


def _is_tensor(v):
    return hasattr(v, "is_cuda") and hasattr(v, "dim")


class SummaryWriter(object):
    """``tf.summary.create_file_writer(logdir)``: ``<logdir>/events.out.tfevents.<seconds>.<host>.<pid>.v2``, opened (with its version
    record) at construction.  ``scalar`` takes a number or a 0-dim tensor; a tensor is NOT read when it is given: events queue in call
    order, and ``flush()`` reads every pending tensor in one stacked transfer per device, then writes the queue.  clock: the source of
    ``wall_time`` (tests)."""

    def __init__(self, logdir, clock=time.time):
        os.makedirs(logdir, exist_ok=True)
        self.clock = clock
        now = clock()
        self.path = os.path.join(logdir, "events.out.tfevents.%010d.%s.%d.v2" % (int(now), socket.gethostname(), os.getpid()))
        self._file = open(self.path, "ab")
        self._file.write(frame_record(encode_event(now, file_version=FILE_VERSION)))
        self._file.flush()
        self._pending = []  # (wall_time, step, tag, number | tensor | image dict)

    def _queue(self, tag, value, step):
        if self._file is None:
            raise ValueError("the writer is closed")
        if not isinstance(tag, str):
            raise ValueError("tag must be a string")
        self._pending.append((self.clock(), int(step), tag, value))

    def scalar(self, tag, value, step):
        if _is_tensor(value):
            if value.numel() != 1:
                raise ValueError("scalar %r: a tensor of %d elements" % (tag, value.numel()))
            value = value.detach().reshape(())
        else:
            value = float(value)
        self._queue(tag, value, step)

    def image(self, tag, frame_or_png_bytes, step):
        """PNG bytes as they are (the header gives height, width and colorspace), or one uint8 frame [H,W,C] / [H,W] on the device,
        encoded here (``encode_png_batch``: this waits for the device)."""
        from .png import png_info

        data = frame_or_png_bytes
        if _is_tensor(data):
            from .png_encode import encode_png_batch

            data = encode_png_batch([data])[0]
        elif not isinstance(data, (bytes, bytearray, memoryview)):
            raise ValueError("image %r: PNG bytes or a uint8 device tensor, not %s" % (tag, type(data).__name__))
        data = bytes(data)
        info = png_info(data)
        self._queue(tag, {"height": info["height"], "width": info["width"], "colorspace": info["samples"], "encoded_image_string": data}, step)

    def flush(self):
        """one device read for all pending tensors (per device), then every queued event to the file, in call order"""
        if self._file is None:
            return
        tensors = [i for i, p in enumerate(self._pending) if _is_tensor(p[3])]
        if tensors:
            import torch

            by_dev = {}
            for i in tensors:
                by_dev.setdefault(self._pending[i][3].device, []).append(i)
            for idx in by_dev.values():
                host = torch.stack([self._pending[i][3].float() for i in idx]).cpu().numpy()
                for i, v in zip(idx, host.tolist()):
                    self._pending[i] = self._pending[i][:3] + (v,)
        for wall, step, tag, value in self._pending:
            self._file.write(frame_record(encode_event(wall, step, [(tag, value)])))
        self._pending = []
        self._file.flush()

    def close(self):
        if self._file is not None:
            self.flush()
            self._file.close()
            self._file = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

