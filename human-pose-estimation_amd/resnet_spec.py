"""ResNet-50 v1 conv-layer table for the encoder the reference instantiates with
``tensorflow.keras.applications.ResNet50(include_top=False, pooling='avg')``
(reference: src/models.py:35-41; topology per SURVEY.md §8(a) row 1).

This is the canonical layer ORDER of the C-ABI (``include/hpe.h``: ``hpe_load_conv`` takes the index
into this table).  Layer names are the Keras ones (``conv1``, ``res2a_branch2a`` … with the matching
``bn*`` BatchNorm), so a Keras-layout weight dict keyed by layer name maps 1:1.

Each entry: (name, bn_name, KH, KW, Cin, Cout, stride, Hin, Hout).
"""
from __future__ import annotations

from collections import namedtuple

ConvSpec = namedtuple("ConvSpec", "name bn_name kh kw cin cout stride hin hout")

STAGE_BLOCKS = {2: 3, 3: 4, 4: 6, 5: 3}
STAGE_FILTERS = {2: (64, 64, 256), 3: (128, 128, 512), 4: (256, 256, 1024), 5: (512, 512, 2048)}


def resnet50_conv_specs():
    specs = [ConvSpec("conv1", "bn_conv1", 7, 7, 3, 64, 2, 224, 112)]
    cin, h = 64, 56  # after 3x3/2 max-pool
    for stage in (2, 3, 4, 5):
        f1, f2, f3 = STAGE_FILTERS[stage]
        for b in range(STAGE_BLOCKS[stage]):
            blk = "abcdef"[b]
            first = b == 0
            s = 2 if (first and stage > 2) else 1
            hout = h // s
            base = "res%d%s_branch" % (stage, blk)
            bn = "bn%d%s_branch" % (stage, blk)
            specs.append(ConvSpec(base + "2a", bn + "2a", 1, 1, cin, f1, s, h, hout))
            specs.append(ConvSpec(base + "2b", bn + "2b", 3, 3, f1, f2, 1, hout, hout))
            specs.append(ConvSpec(base + "2c", bn + "2c", 1, 1, f2, f3, 1, hout, hout))
            if first:
                specs.append(ConvSpec(base + "1", bn + "1", 1, 1, cin, f3, s, h, hout))
            cin, h = f3, hout
    return specs


CONV_SPECS = resnet50_conv_specs()
CONV_INDEX = {s.name: i for i, s in enumerate(CONV_SPECS)}


def encoder_param_count():
    n = 0
    for s in CONV_SPECS:
        n += s.kh * s.kw * s.cin * s.cout + s.cout  # kernel + bias
        n += 4 * s.cout  # BN gamma, beta, moving_mean, moving_variance
    return n


# ---- the flat layout of the trainable encoder parameters (include/hpe.h: hpe_encoder_param_offset): per layer kernel HWIO, bias, gamma, beta
PARAM_PARTS = ("kernel", "bias", "gamma", "beta")


def encoder_param_offsets():
    """[(kernel, bias, gamma, beta offsets)] per layer and the total float count"""
    offs, o = [], 0
    for s in CONV_SPECS:
        kn = s.kh * s.kw * s.cin * s.cout
        offs.append((o, o + kn, o + kn + s.cout, o + kn + 2 * s.cout))
        o += kn + 3 * s.cout
    return offs, o


ENCODER_PARAM_OFFSETS, ENCODER_PARAM_FLOATS = encoder_param_offsets()


def _flat_keys(s):
    return (s.name + "/kernel", s.name + "/bias", s.bn_name + "/gamma", s.bn_name + "/beta")


def params_to_flat(params):
    """the dict ``load_encoder`` takes -> the flat float32 array (the statistics are not in it)"""
    import numpy as np

    out = np.empty(ENCODER_PARAM_FLOATS, np.float32)
    for s, off in zip(CONV_SPECS, ENCODER_PARAM_OFFSETS):
        for key, o in zip(_flat_keys(s), off):
            v = np.asarray(params[key], np.float32).reshape(-1)
            out[o:o + v.size] = v
    return out


def flat_to_params(flat, stats):
    """flat array (or CPU/CUDA tensor) -> the dict ``load_encoder`` takes; moving_mean / moving_variance are passed through from ``stats``
    (any dict that holds them, e.g. the parameters the flat array came from)"""
    import numpy as np

    if hasattr(flat, "detach"):
        flat = flat.detach().cpu().numpy()
    flat = np.asarray(flat, np.float32).reshape(-1)
    if flat.size != ENCODER_PARAM_FLOATS:
        raise ValueError("flat must hold %d floats, got %d" % (ENCODER_PARAM_FLOATS, flat.size))
    out = {}
    for s, off in zip(CONV_SPECS, ENCODER_PARAM_OFFSETS):
        shapes = ((s.kh, s.kw, s.cin, s.cout), (s.cout,), (s.cout,), (s.cout,))
        for key, o, shp in zip(_flat_keys(s), off, shapes):
            out[key] = flat[o:o + int(np.prod(shp))].reshape(shp).copy()
        for k in ("/moving_mean", "/moving_variance"):
            out[s.bn_name + k] = np.asarray(stats[s.bn_name + k], np.float32)
    return out


# ---- the layout of the moving statistics (include/hpe.h: hpe_encoder_stat_offset): moving_mean of every layer, then moving_variance of
# every layer, both in table order
ENCODER_STAT_CHANNELS = sum(s.cout for s in CONV_SPECS)
ENCODER_STAT_FLOATS = 2 * ENCODER_STAT_CHANNELS


def encoder_stat_offsets():
    """[(moving_mean offset, moving_variance offset)] per layer"""
    offs, o = [], 0
    for s in CONV_SPECS:
        offs.append((o, ENCODER_STAT_CHANNELS + o))
        o += s.cout
    return offs


ENCODER_STAT_OFFSETS = encoder_stat_offsets()


def params_to_stats(params):
    """the dict ``load_encoder`` takes -> its moving statistics as the flat float32 array of ``HpeEngine.encoder_stats``"""
    import numpy as np

    out = np.empty(ENCODER_STAT_FLOATS, np.float32)
    for s, (om, ov) in zip(CONV_SPECS, ENCODER_STAT_OFFSETS):
        out[om:om + s.cout] = np.asarray(params[s.bn_name + "/moving_mean"], np.float32).reshape(-1)
        out[ov:ov + s.cout] = np.asarray(params[s.bn_name + "/moving_variance"], np.float32).reshape(-1)
    return out


def stats_to_params(stats):
    """the flat statistics (array or CPU/CUDA tensor) -> {bn_name/moving_mean, bn_name/moving_variance}: what ``flat_to_params`` takes as
    its ``stats``, so ``flat_to_params(trainer.encoder_params, stats_to_params(trainer.encoder_stats))`` is a trained encoder, whole"""
    import numpy as np

    if hasattr(stats, "detach"):
        stats = stats.detach().cpu().numpy()
    stats = np.asarray(stats, np.float32).reshape(-1)
    if stats.size != ENCODER_STAT_FLOATS:
        raise ValueError("stats must hold %d floats, got %d" % (ENCODER_STAT_FLOATS, stats.size))
    out = {}
    for s, (om, ov) in zip(CONV_SPECS, ENCODER_STAT_OFFSETS):
        out[s.bn_name + "/moving_mean"] = stats[om:om + s.cout].copy()
        out[s.bn_name + "/moving_variance"] = stats[ov:ov + s.cout].copy()
    return out


def encoder_macs_per_image():
    return sum(s.kh * s.kw * s.cin * s.cout * s.hout * s.hout for s in CONV_SPECS)


def encoder_min_bytes_per_image(elem_bytes=4):
    """Algorithmic HBM bytes of the encoder per image when every activation tensor is written once and read once
    by each consumer (no on-chip fusion across layers): conv inputs actually touched (1x1/s2 convs read one pixel
    in four), conv outputs, residual reads of the 2c layers, the two pools; plus the fp32 input image and its padded
    copy.  Weights (read once per batch) are not included."""
    total = 224 * 224 * 3 * 4  # fp32 image read by the pad kernel
    total += 2 * 230 * 232 * 4 * elem_bytes  # padded copy written + read by conv1
    for s in CONV_SPECS:
        if s.name == "conv1":
            total += s.hout * s.hout * s.cout * elem_bytes  # conv1 out
            total += s.hout * s.hout * s.cout * elem_bytes + 56 * 56 * 64 * elem_bytes  # max-pool read + write
            continue
        total += s.hout * s.hout * s.cin * elem_bytes  # input pixels touched once (3x3 taps re-read from L2)
        total += s.hout * s.hout * s.cout * elem_bytes  # output
        if s.name.endswith("2c"):
            total += s.hout * s.hout * s.cout * elem_bytes  # residual
    total += 7 * 7 * 2048 * elem_bytes + 2048 * 4  # avg-pool
    return total
