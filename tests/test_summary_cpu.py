"""CPU tests of the event files (no GPU): the byte-exact payload of one scalar event; a written file read back through
``read_tfrecords(verify=True)`` and ``read_events``; image values round-trip; scalars given as tensors do not reach the file before
``flush()``; a corrupted CRC is refused; and the hooks of ``run_training_loop`` fire at the reference's steps."""
import os
import re
import struct

import numpy as np
import pytest
import torch

import hpe_amd
from hpe_amd import summary
from hpe_amd.trainer import run_training_loop

import png_encode_ref as E


def test_scalar_event_payload_is_byte_exact():
    want = bytes.fromhex("09 00 00 00 00 00 00 f8 3f 10 03 2a 0a 0a 08 0a 01 61 15 00 00 80 3e")
    assert summary.encode_event(1.5, 3, [("a", 0.25)]) == want
    assert summary.decode_event(want) == {"wall_time": 1.5, "step": 3, "values": [{"tag": "a", "simple_value": 0.25}]}


def test_defaults_are_omitted_and_the_oneof_is_kept():
    assert summary.encode_event(0.0, 0) == b""  # proto3: zero scalars are not written
    assert summary.encode_event(2.0, 0, [("t", 0.0)]) == bytes.fromhex("09 00 00 00 00 00 00 00 40 2a 0a 0a 08 0a 01 74 15 00 00 00 00")
    assert summary.encode_event(1.0, file_version="brain.Event:2") == b"\x09" + struct.pack("<d", 1.0) + b"\x1a\x0dbrain.Event:2"
    assert summary.decode_event(summary.encode_event(1.0, -2, [("t", -1.5)]))["step"] == -2  # int64: ten varint bytes


def test_file_reads_back(tmp_path):
    ticks = iter(np.arange(100.0, 200.0, 0.5).tolist())
    w = hpe_amd.SummaryWriter(str(tmp_path / "training"), clock=lambda: next(ticks))
    assert re.fullmatch(r"events\.out\.tfevents\.0000000100\.[^/]+\.%d\.v2" % os.getpid(), os.path.basename(w.path))
    w.scalar("generator/kpr_loss", 0.5, 1)
    w.scalar("critic/penalty", np.float32(3.25), 1)
    w.scalar("generator/kpr_loss", 0.125, 2)
    w.close()
    w.close()  # twice is fine
    payloads = list(hpe_amd.read_tfrecords(w.path, verify=True))
    assert len(payloads) == 4 and payloads[0] == summary.encode_event(100.0, file_version="brain.Event:2")
    ev = hpe_amd.read_events(w.path)
    assert ev[0] == {"wall_time": 100.0, "step": 0, "values": [], "file_version": "brain.Event:2"}
    assert [(e["wall_time"], e["step"], e["values"][0]["tag"], e["values"][0]["simple_value"]) for e in ev[1:]] == [
        (100.5, 1, "generator/kpr_loss", 0.5), (101.0, 1, "critic/penalty", 3.25), (101.5, 2, "generator/kpr_loss", 0.125)]
    with pytest.raises(ValueError, match="closed"):
        w.scalar("a", 1.0, 3)


def test_image_values_round_trip(tmp_path):
    frames = [E.content(5, 7, 1, 0), E.content(17, 13, 3, 1), E.content(4, 6, 4, 2)]
    streams = [E.encode(f) for f in frames]
    with hpe_amd.SummaryWriter(str(tmp_path)) as w:
        for i, s in enumerate(streams):
            w.image("vis_images/%d" % i, s, 7)
        with pytest.raises(hpe_amd.HpeError, match="signature"):
            w.image("bad", b"not a png", 7)
        with pytest.raises(ValueError, match="PNG bytes"):
            w.image("bad", frames[0], 7)  # a host array is neither
    ev = hpe_amd.read_events(w.path)[1:]
    assert len(ev) == 3
    for i, (e, f, s) in enumerate(zip(ev, frames, streams)):
        assert e["step"] == 7 and len(e["values"]) == 1 and e["values"][0]["tag"] == "vis_images/%d" % i
        assert e["values"][0]["image"] == {"height": f.shape[0], "width": f.shape[1], "colorspace": f.shape[2], "encoded_image_string": s}


def test_tensor_scalars_wait_for_flush(tmp_path):
    w = hpe_amd.SummaryWriter(str(tmp_path))
    size = os.path.getsize(w.path)
    assert len(hpe_amd.read_events(w.path)) == 1  # the version record is there from the start
    a, b = torch.tensor(0.75), torch.tensor([[2.5]])
    w.scalar("x", a, 1)
    w.scalar("y", 1.0, 1)
    w.scalar("x", b, 2)
    assert os.path.getsize(w.path) == size  # nothing reached the file, the number queued behind the tensor included
    a.fill_(0.5)  # not read yet: flush sees the value the tensor holds then
    w.flush()
    got = [(e["step"], e["values"][0]["tag"], e["values"][0]["simple_value"]) for e in hpe_amd.read_events(w.path)[1:]]
    assert got == [(1, "x", 0.5), (1, "y", 1.0), (2, "x", 2.5)]
    with pytest.raises(ValueError, match="2 elements"):
        w.scalar("z", torch.zeros(2), 3)
    w.close()


def test_a_corrupted_crc_is_refused(tmp_path):
    with hpe_amd.SummaryWriter(str(tmp_path)) as w:
        w.scalar("a", 1.0, 1)
    data = bytearray(open(w.path, "rb").read())
    data[-6] ^= 0x40  # inside the last payload
    bad = tmp_path / "bad.v2"
    bad.write_bytes(bytes(data))
    with pytest.raises(hpe_amd.RecordError, match="record 1: the CRC of the payload"):
        hpe_amd.read_events(str(bad))
    data = bytearray(open(w.path, "rb").read())
    data[9] ^= 1  # the CRC of the first length
    bad.write_bytes(bytes(data))
    with pytest.raises(hpe_amd.RecordError, match="record 0: the CRC of the length"):
        hpe_amd.read_events(str(bad))


def test_hooks_fire_at_the_references_steps():
    """after every train step with the 1-based step; after a validation step when step % validation_step_size == 0, following that
    step's train hook (src/trainer.py:745-809); the epoch hook when the epoch rolls.  Without hooks the loop's result is the same."""
    calls = []
    kw = dict(num_images=6, batch_size=2, max_epoch=2, validation_step_size=2, log=lambda s: None)
    batches = lambda: ((i, -i, 10 * i) for i in range(1, 100))  # noqa: E731
    out = run_training_loop(batches(), lambda g, c: ("train", g, c), val_step=lambda v: ("val", v),
                            after_train_step=lambda s, r: calls.append(("t", s, r)), after_val_step=lambda s, r: calls.append(("v", s, r)),
                            after_epoch=lambda e: calls.append(("e", e)), **kw)
    assert calls == [("t", 1, ("train", 1, -1)), ("t", 2, ("train", 2, -2)), ("v", 2, ("val", 20)), ("t", 3, ("train", 3, -3)), ("e", 0),
                     ("t", 4, ("train", 4, -4)), ("v", 4, ("val", 40)), ("t", 5, ("train", 5, -5)), ("t", 6, ("train", 6, -6)),
                     ("v", 6, ("val", 60)), ("e", 1)]
    assert out == run_training_loop(batches(), lambda g, c: None, val_step=lambda v: None, **kw) == {"steps": 6, "epochs": 2, "saved": [], "validations": 3}
