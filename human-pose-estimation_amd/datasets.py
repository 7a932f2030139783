"""Dataset writers: the reference's ``create_datasets.py`` and ``src/util/create_dataset.py`` without TensorFlow or scipy -- raw LSP,
LSP-extended and MPII folders become the ``*.tfrecords`` files the reader of records.py and the trainers take.  The records are the
reference's: image bytes as they are, the mask re-encoded as a one-channel JPEG for LSP-extended and MPII (``encode_jpeg_batch`` at
its defaults, which is ``tf.image.encode_jpeg``'s stream byte for byte), visibility, centre and face points by the reference's rules.
Only the mask re-encode touches the device; it is batched.  DESIGN.md "Dataset writers and JPEG encode"."""
from __future__ import annotations

import os
import re
from glob import glob

import numpy as np

from . import mat5_lite
from ._lib import HpeError
from .records import TFRecordWriter, image_example

DATASETS = ("lsp", "lsp_ext", "mpii")
# src/util/create_dataset.py:109-125: MPII's joints in LSP's order (R ankle .. L ankle, R wrist .. L wrist, neck top, head top)
MPII_TO_LSP = (0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 8, 9)
LSP_TRAIN = 1000  # create_datasets.py:15, 20: the first 1000 pairs train, the rest validate


def _pairs(images, segs, what):
    if len(images) != len(segs):
        raise ValueError("%s: %d images but %d segmentations" % (what, len(images), len(segs)))
    return list(zip(images, segs))


def _number(path):
    """the number in a file's base name (im0001.jpg, im00001_segmentation.png, 00001.png).  The reference takes the first or second
    number of the whole path, which under its own directory layout is this one."""
    found = re.findall(r"\d+", os.path.basename(path))
    if not found:
        raise ValueError("%s: no number in the file name" % path)
    return int(found[0])


def filename_pairs_lsp(im_dir, seg_dir):
    """create_dataset.py:144-149: every ``*.jpg`` with ``imNNNN_segmentation.png``, both sorted, paired by position"""
    images = sorted(glob(os.path.join(im_dir, "*.jpg")))
    segs = sorted(glob(os.path.join(seg_dir, "im[0-9][0-9][0-9][0-9]_segmentation.png")))
    return _pairs(images, segs, "lsp")


def filename_pairs_lspe(im_dir, seg_dir):
    """create_dataset.py:151-163: only some frames have a mask: mask number n goes with the n-th image (1-based) of the sorted list"""
    images = sorted(glob(os.path.join(im_dir, "*.jpg")))
    segs = sorted(glob(os.path.join(seg_dir, "im[0-9][0-9][0-9][0-9][0-9]_segmentation.png")))
    picked = []
    for s in segs:
        n = _number(s)
        if not 1 <= n <= len(images):
            raise ValueError("lsp_ext: %s has number %d, there are %d images" % (s, n, len(images)))
        picked.append(images[n - 1])
    return _pairs(picked, segs, "lsp_ext")


def filename_pairs_mpii(mpii_dir):
    """create_dataset.py:165-170: ``images/NNNNN.png`` with ``images/NNNNN_segmentation.png``, both sorted, paired by position"""
    d = os.path.join(mpii_dir, "images")
    images = sorted(glob(os.path.join(d, "[0-9][0-9][0-9][0-9][0-9].png")))
    segs = sorted(glob(os.path.join(d, "[0-9][0-9][0-9][0-9][0-9]_segmentation.png")))
    return _pairs(images, segs, "mpii")


def load_labels(labels, dataset):
    """labels -> float64 [3, K, N]: an array, a ``.npz`` (key 'poses'), or a MATLAB v5 ``.mat`` (variable 'joints', through mat5_lite).
    MPII's 16 joints are reordered to LSP's 14 (``MPII_TO_LSP``); an array whose first axis is not 3 has its first two axes swapped
    (create_dataset.py:125-128)."""
    if dataset not in DATASETS:
        raise ValueError("dataset must be one of %s" % (DATASETS,))
    if isinstance(labels, (str, bytes, os.PathLike)):
        path = os.fspath(labels)
        if str(path).endswith(".npz"):
            with np.load(path) as z:
                if "poses" not in z.files:
                    raise ValueError("%s holds no 'poses'" % path)
                labels = z["poses"]
        else:
            mat = mat5_lite.load(path)
            if "joints" not in mat:
                raise ValueError("%s holds no 'joints' (it holds %s)" % (path, sorted(mat)))
            labels = mat["joints"]
    arr = np.array(labels, dtype=np.float64)
    if arr.ndim != 3:
        raise ValueError("labels must have 3 axes, got shape %s" % (arr.shape,))
    if dataset == "mpii":
        arr = arr[:, MPII_TO_LSP, :]
    if arr.shape[0] != 3:
        arr = np.transpose(arr, (1, 0, 2))
    if arr.shape[0] != 3:
        raise ValueError("labels must be [3, K, N] or [K, 3, N], got shape %s" % (arr.shape,))
    return arr


def _size(data, path):
    """(height, width) from the stream's header alone: SOF0 of a JPEG, IHDR of a PNG"""
    from .jpeg import jpeg_info
    from .png import png_info, sniff

    kind = sniff(data)
    if kind is None:
        raise HpeError("%s: neither a JPEG nor a PNG stream" % path)
    info = jpeg_info(data) if kind == "jpeg" else png_info(data)
    return info["height"], info["width"]


def _own_channels(data, path):
    """the channel count ``tf.image.decode_jpeg(data)`` gives with channels=0: 1 for a grey stream, else 3 (alpha is dropped)"""
    from .jpeg import jpeg_info
    from .png import png_info, sniff

    kind = sniff(data)
    if kind is None:
        raise HpeError("%s: neither a JPEG nor a PNG stream" % path)
    if kind == "jpeg":
        return 1 if jpeg_info(data)["components"] == 1 else 3
    return 1 if png_info(data)["color_type"] in (0, 4) else 3


def record_fields(img_path, seg_path, label, dataset):
    """create_dataset.py:17-50 but for the mask re-encode: -> dict of ``image_example``'s arguments, 'seg' still the file's bytes.
    label float [3, 14] or [3, 19] (x, y, flag), not modified.  LSP-extended's flag IS the visibility; LSP's and MPII's is its negation."""
    if dataset not in DATASETS:
        raise ValueError("dataset must be one of %s" % (DATASETS,))
    label = np.array(label, dtype=np.float64)
    if label.ndim != 2 or label.shape[0] != 3 or label.shape[1] not in (14, 19):
        raise ValueError("%s: label must be [3, 14] or [3, 19], got %s" % (img_path, label.shape))
    if dataset == "lsp_ext":
        visible = label[2].astype(bool)
    else:
        visible = np.logical_not(label[2])
        label[2] = visible.astype(label.dtype)
    if not visible.any():
        raise ValueError("%s: no visible joint: the centre is undefined" % img_path)
    center = ((label[:2, visible].min(axis=1) + label[:2, visible].max(axis=1)) / 2.0).astype(np.int64)  # truncated, as astype(int)
    with open(img_path, "rb") as f:
        image = f.read()
    with open(seg_path, "rb") as f:
        seg = f.read()
    height, width = _size(image, img_path)
    face = label[:, 14:].ravel() if label.shape[1] == 19 else None  # the face points go in on their own, 3 x 5
    label = label[:, :14]
    return {"image": image, "seg": seg, "height": height, "width": width, "center": center, "filename": os.path.basename(os.fspath(img_path)),
            "x": label[0], "y": label[1], "vis": label[2].astype(np.int64), "face_pts": face}


def reencode_masks(masks, paths, threads=8):
    """create_dataset.py:36-40 for a batch: every mask stream decoded with its own channel count, channel 0 kept, and that one channel
    encoded as a JPEG at ``encode_jpeg_batch``'s defaults -> list[bytes].  Two decodes at most (the grey masks, the colour masks), one
    encode launch."""
    from .jpeg_encode import encode_jpeg_batch
    from .png import decode_image_batch

    counts = [_own_channels(m, p) for m, p in zip(masks, paths)]
    planes = [None] * len(masks)
    for ch in (1, 3):
        idx = [i for i, c in enumerate(counts) if c == ch]
        if not idx:
            continue
        for i, frame in zip(idx, decode_image_batch([masks[i] for i in idx], channels=ch, threads=threads).frames):
            planes[i] = frame if ch == 1 else frame[:, :, 0].contiguous()
    return encode_jpeg_batch(planes, threads=threads)


def image_record(img_path, seg_path, label, dataset):
    """One pair -> the serialized ``tf.train.Example`` of create_dataset.py:17-72"""
    f = record_fields(img_path, seg_path, label, dataset)
    if dataset != "lsp":
        f["seg"] = reencode_masks([f["seg"]], [seg_path])[0]
    return image_example(**f)


def create_records(path, pairs, labels, dataset, batch=64, threads=8):
    """create_dataset.py:90-142: one record per (image, mask) pair into ``path``; pair i takes column ``number - 1`` of ``labels``
    ([3, K, N], or what ``load_labels`` takes), ``number`` being the one in the image's file name.  The mask re-encodes of LSP-extended
    and MPII run ``batch`` at a time.  -> the number of records written."""
    labels = load_labels(labels, dataset)
    if int(batch) < 1:
        raise ValueError("batch must be >= 1")
    with TFRecordWriter(path) as w:
        for start in range(0, len(pairs), int(batch)):
            fields = []
            for img, seg in pairs[start:start + int(batch)]:
                n = _number(img)
                if not 1 <= n <= labels.shape[2]:
                    raise ValueError("%s has number %d, the labels hold %d columns" % (img, n, labels.shape[2]))
                fields.append(record_fields(img, seg, labels[:, :, n - 1], dataset))
            if dataset != "lsp" and fields:
                segs = reencode_masks([f["seg"] for f in fields], [seg for _, seg in pairs[start:start + int(batch)]], threads)
                for f, s in zip(fields, segs):
                    f["seg"] = s
            for f in fields:
                w.write(image_example(**f))
        return w.count


def create_datasets(config):
    """create_datasets.py:12-31.  ``config`` carries the reference's flags as attributes: ``dataset_dir`` (where the files go),
    ``create_lsp`` / ``create_lsp_val`` / ``create_lsp_ext`` / ``create_mpii``, ``lsp_dir`` / ``lsp_im`` / ``lsp_seg``,
    ``lsp_e_dir`` / ``lsp_e_im`` / ``lsp_e_seg``, ``mpii_dir`` / ``mpii_poses_dir``; the labels are ``joints.mat`` of ``lsp_dir`` and
    ``lsp_e_dir`` and ``poses.npz``.  -> {file path: records written}."""
    out = {}
    os.makedirs(config.dataset_dir, exist_ok=True)
    target = lambda name: os.path.join(config.dataset_dir, name)  # noqa: E731
    if getattr(config, "create_lsp", False) or getattr(config, "create_lsp_val", False):
        pairs = filename_pairs_lsp(config.lsp_im, config.lsp_seg)
        labels = os.path.join(config.lsp_dir, "joints.mat")
        if getattr(config, "create_lsp", False):
            out[target("lsp_train.tfrecords")] = create_records(target("lsp_train.tfrecords"), pairs[:LSP_TRAIN], labels, "lsp")
        if getattr(config, "create_lsp_val", False):
            out[target("lsp_val.tfrecords")] = create_records(target("lsp_val.tfrecords"), pairs[LSP_TRAIN:], labels, "lsp")
    if getattr(config, "create_lsp_ext", False):
        pairs = filename_pairs_lspe(config.lsp_e_im, config.lsp_e_seg)
        out[target("lsp_ext.tfrecords")] = create_records(target("lsp_ext.tfrecords"), pairs, os.path.join(config.lsp_e_dir, "joints.mat"), "lsp_ext")
    if getattr(config, "create_mpii", False):
        pairs = filename_pairs_mpii(config.mpii_dir)
        out[target("mpii.tfrecords")] = create_records(target("mpii.tfrecords"), pairs, config.mpii_poses_dir, "mpii")
    return out
