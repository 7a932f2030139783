"""Stand-alone reader and writer for the TensorFlow-2 object-graph checkpoints the reference restores its weights from
 -- no TensorFlow involved.

What the reference does (src/predictor.py:77-86, same in src/trainer.py:192-198,836):

    checkpoint = tf.train.Checkpoint(generator_optimizer=..., discriminator_optimizer=...,
                                     feature_extractor=<Keras ResNet50>, generator3d=<Sequential of 3 Dense>,
                                     discriminator=..., inital_theta=<Variable [1,85]>)
    checkpoint.restore(tf.train.latest_checkpoint(checkpoint_dir)).expect_partial()

On disk that is ``<dir>/checkpoint`` (a text file naming the newest prefix) plus a *TensorBundle*
``ckpt-N.index`` / ``ckpt-N.data-00000-of-00001``:

  * the index is a LevelDB-format sorted string table: data blocks of prefix-compressed key/value entries with a
    restart array, each block followed by a 1-byte compression tag and a masked CRC-32C; a 48-byte footer holds the
    handles of the meta-index and index blocks and the magic 0xdb4775248b80fb57;
  * key "" -> BundleHeaderProto (num_shards, endianness); every other key -> BundleEntryProto
    (dtype, shape, shard_id, offset, size, masked crc32c) pointing into a data shard of raw little-endian tensors;
  * key ``_CHECKPOINTABLE_OBJECT_GRAPH`` is a string tensor holding a TrackableObjectGraph proto: the tree of
    Python attribute names (``feature_extractor`` -> ``layer_with_weights-3`` -> ``kernel``) with, per variable, its
    ``full_name`` (the Keras variable name, e.g. ``res2a_branch2a/kernel``) and its ``checkpoint_key``.

``load_hmr_weights`` (encoder, regressor) and ``load_critic_weights`` (the ``discriminator``) walk that graph, so Keras layer names -- not positional guesses -- decide which tensor feeds
which ``hpe_load_conv`` / ``hpe_load_dense`` slot; when a checkpoint has no graph entry the positional order of
keras_applications 1.0.8 / tf.keras >= 2.2 is used and cross-checked against every kernel shape.

PARITY UNPINNED: no TensorFlow-written checkpoint exists in this environment (the trained weights are "contact the
authors", README.md:76) -- the reader follows the published formats (LevelDB table_format.md; tensor_bundle.proto;
trackable_object_graph.proto) and is tested against bundles produced by the independent writer in
tests/tf_bundle_writer.py.

The second half of this file is the writer of the same layout (``save_checkpoint``, ``write_bundle``) and ``load_training_state``, which
reads the optimisers' step counts and moments back; its parity with TensorFlow is unpinned in the same way (see its header below).
"""
from __future__ import annotations

import os
import re

import numpy as np

from .critic_spec import CRITIC_LAYERS
from .resnet_spec import CONV_SPECS

TABLE_MAGIC = 0xDB4775248B80FB57
OBJECT_GRAPH_KEY = "_CHECKPOINTABLE_OBJECT_GRAPH"
VAR_SUFFIX = "/.ATTRIBUTES/VARIABLE_VALUE"

_DTYPES = {1: "<f4", 2: "<f8", 3: "<i4", 4: "u1", 5: "<i2", 6: "i1", 9: "<i8", 10: "?", 17: "<u2", 19: "<f2", 22: "<u4", 23: "<u8"}
DT_STRING = 7


class CheckpointError(ValueError):
    pass


def _guard(fn):
    """A damaged index (bad UTF-8 in a key, a field with the wrong wire type, lengths past the end ...) surfaces as
    CheckpointError, never as a stray exception type."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **k):
        try:
            return fn(*a, **k)
        except (CheckpointError, FileNotFoundError, KeyError):
            raise
        except (ValueError, TypeError, IndexError, OverflowError, MemoryError, UnicodeError) as e:
            raise CheckpointError("corrupt checkpoint structure: %s: %s" % (type(e).__name__, e)) from e

    return wrapped


# ----------------------------------------------------------------------------------------------- CRC-32C (Castagnoli)
def _crc_table():
    t = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t[i] = c
    return t


_CRC_NP = _crc_table()
_CRC_T = [int(x) for x in _CRC_NP]


def _crc_bytewise(data, state):
    t = _CRC_T
    for b in bytes(data):
        state = t[(state ^ b) & 0xFF] ^ (state >> 8)
    return state


def _mat_apply(cols, v):
    """GF(2) 32x32 matrix (32 uint32 columns) times vector(s): xor of the columns selected by the bits of v."""
    if isinstance(v, np.ndarray):
        out = np.zeros_like(v)
        for bit in range(32):
            out ^= np.where((v >> np.uint32(bit)) & np.uint32(1), np.uint32(cols[bit]), np.uint32(0)).astype(np.uint32)
        return out
    out = 0
    for bit in range(32):
        if (v >> bit) & 1:
            out ^= cols[bit]
    return out


def _mat_square(cols):
    return [_mat_apply(cols, c) for c in cols]


_ZERO_BYTE = [_crc_bytewise(b"\0", 1 << bit) for bit in range(32)]  # register update for one zero byte, as a matrix


_SHIFT_POW2 = [_ZERO_BYTE]  # [k] = matrix advancing the register over 2^k zero bytes


def _shift_pow2(k):
    while len(_SHIFT_POW2) <= k:
        _SHIFT_POW2.append(_mat_square(_SHIFT_POW2[-1]))
    return _SHIFT_POW2[k]


_CRC_NP16 = None


def _crc_table16():
    """[x] = the register after the two bytes x & 0xFF, x >> 8 from a register of zero: one lookup advances a lane by two bytes"""
    global _CRC_NP16
    if _CRC_NP16 is None:
        x = np.arange(65536, dtype=np.uint32)
        r = _CRC_NP[x & np.uint32(0xFF)] ^ (x >> np.uint32(8))
        _CRC_NP16 = _CRC_NP[r & np.uint32(0xFF)] ^ (r >> np.uint32(8))
    return _CRC_NP16


def crc32c(data, crc=0):
    """CRC-32C (Castagnoli, reflected 0x82F63B78).  Large buffers use the register's linearity over GF(2): the initial
    register value is folded into the first four bytes, the buffer is zero-padded at the FRONT (a zero register stays
    zero over zero bytes) to lanes x L bytes, all lanes advance in lock-step with one vectorised table lookup per byte
    column, and lanes are merged pairwise with the zero-byte shift matrices of 2^k bytes."""
    if isinstance(data, np.ndarray):
        a = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    else:
        a = np.frombuffer(bytes(data), dtype=np.uint8)
    n = a.shape[0]
    init = (crc ^ 0xFFFFFFFF) & 0xFFFFFFFF
    if n < 8192:
        return _crc_bytewise(a.tobytes(), init) ^ 0xFFFFFFFF
    logL = 8 if n < (1 << 19) else (10 if n < (1 << 23) else 12)
    L = 1 << logL
    lanes = 1
    while lanes * L < n:
        lanes *= 2
    buf = np.zeros(lanes * L, dtype=np.uint8)
    buf[lanes * L - n:] = a
    head = buf[lanes * L - n:lanes * L - n + 4]
    head ^= np.frombuffer(init.to_bytes(4, "little"), dtype=np.uint8)
    cols = np.ascontiguousarray(buf.reshape(lanes, L).view("<u2").T)  # two bytes per step (the table of _crc_table16)
    reg = np.zeros(lanes, dtype=np.uint32)
    t16, m16, s16 = _crc_table16(), np.uint32(0xFFFF), np.uint32(16)
    for j in range(L // 2):
        reg = t16[(reg ^ cols[j]) & m16] ^ (reg >> s16)
    k = logL
    while reg.shape[0] > 1:
        reg = _mat_apply(_shift_pow2(k), reg[0::2]) ^ reg[1::2]
        k += 1
    return int(reg[0]) ^ 0xFFFFFFFF


def mask_crc(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


# ----------------------------------------------------------------------------------------------- varints / protobuf wire format
def _varint(buf, pos):
    shift = result = 0
    while True:
        if pos >= len(buf):
            raise CheckpointError("truncated varint")
        b = buf[pos]
        pos += 1
        result |= (b & 0x7F) << shift
        if not b & 0x80:
            return result, pos
        shift += 7
        if shift > 70:
            raise CheckpointError("varint too long")


def _proto_fields(buf):
    """Yield (field_number, wire_type, value) -- value is int for varint/fixed, bytes for length-delimited."""
    pos = 0
    while pos < len(buf):
        tag, pos = _varint(buf, pos)
        fn, wt = tag >> 3, tag & 7
        if wt == 0:
            v, pos = _varint(buf, pos)
        elif wt == 1:
            v = int.from_bytes(buf[pos:pos + 8], "little")
            pos += 8
        elif wt == 2:
            n, pos = _varint(buf, pos)
            if pos + n > len(buf):
                raise CheckpointError("truncated protobuf field")
            v = bytes(buf[pos:pos + n])
            pos += n
        elif wt == 5:
            v = int.from_bytes(buf[pos:pos + 4], "little")
            pos += 4
        else:
            raise CheckpointError("unsupported protobuf wire type %d" % wt)
        yield fn, wt, v


def _signed64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


# ----------------------------------------------------------------------------------------------- snappy (block format), decode only
def _snappy_decompress(src):
    n, pos = _varint(src, 0)
    out = bytearray()
    while pos < len(src):
        tag = src[pos]
        pos += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                ln = int.from_bytes(src[pos:pos + nb], "little")
                pos += nb
            ln += 1
            out += src[pos:pos + ln]
            pos += ln
            continue
        if kind == 1:
            ln = ((tag >> 2) & 7) + 4
            off = ((tag >> 5) << 8) | src[pos]
            pos += 1
        elif kind == 2:
            ln = (tag >> 2) + 1
            off = int.from_bytes(src[pos:pos + 2], "little")
            pos += 2
        else:
            ln = (tag >> 2) + 1
            off = int.from_bytes(src[pos:pos + 4], "little")
            pos += 4
        if off == 0 or off > len(out):
            raise CheckpointError("corrupt snappy block")
        for _ in range(ln):  # overlapping copies are legal
            out.append(out[-off])
    if len(out) != n:
        raise CheckpointError("snappy length mismatch")
    return bytes(out)


# ----------------------------------------------------------------------------------------------- sorted string table (.index)
class _Table:
    def __init__(self, buf, verify=True):
        self.buf = buf
        self.verify = verify
        if len(buf) < 48:
            raise CheckpointError("index file too short for a table footer")
        footer = buf[-48:]
        if int.from_bytes(footer[40:], "little") != TABLE_MAGIC:
            raise CheckpointError("not a TensorBundle index (bad table magic)")
        _mo, p = _varint(footer, 0)
        _ms, p = _varint(footer, p)
        io, p = _varint(footer, p)
        isz, p = _varint(footer, p)
        self.index_handle = (io, isz)

    def _block(self, off, size):
        if off + size + 5 > len(self.buf):
            raise CheckpointError("block handle outside the file")
        raw = self.buf[off:off + size]
        ctype = self.buf[off + size]
        stored = int.from_bytes(self.buf[off + size + 1:off + size + 5], "little")
        if self.verify and mask_crc(crc32c(self.buf[off:off + size + 1])) != stored:
            raise CheckpointError("block checksum mismatch at offset %d" % off)
        if ctype == 1:
            raw = _snappy_decompress(raw)
        elif ctype != 0:
            raise CheckpointError("unknown block compression %d" % ctype)
        return raw

    @staticmethod
    def _entries(block):
        if len(block) < 4:
            raise CheckpointError("block too short")
        nrestart = int.from_bytes(block[-4:], "little")
        end = len(block) - 4 - 4 * nrestart
        if end < 0:
            raise CheckpointError("bad restart array")
        pos, key = 0, b""
        while pos < end:
            shared, pos = _varint(block, pos)
            non_shared, pos = _varint(block, pos)
            vlen, pos = _varint(block, pos)
            if shared > len(key) or pos + non_shared + vlen > end:
                raise CheckpointError("corrupt block entry")
            key = key[:shared] + block[pos:pos + non_shared]
            pos += non_shared
            yield key, block[pos:pos + vlen]
            pos += vlen

    def items(self):
        for _k, handle in self._entries(self._block(*self.index_handle)):
            off, p = _varint(handle, 0)
            size, _p = _varint(handle, p)
            yield from self._entries(self._block(off, size))


# ----------------------------------------------------------------------------------------------- TensorBundle
class _Entry:
    __slots__ = ("dtype", "shape", "shard", "offset", "size", "crc", "sliced")


class BundleReader:
    """``BundleReader(prefix)`` -- prefix as given to ``Checkpoint.save`` (``.../ckpt-7``)."""

    @_guard
    def __init__(self, prefix, verify=True):
        self.prefix = str(prefix)
        self.verify = verify
        ipath = self.prefix + ".index"
        if not os.path.exists(ipath):
            raise FileNotFoundError(ipath)
        with open(ipath, "rb") as f:
            table = _Table(f.read(), verify=verify is not False)
        self.entries = {}
        self.num_shards = None
        for k, v in table.items():
            if k == b"":
                for fn, _wt, val in _proto_fields(v):
                    if fn == 1:
                        self.num_shards = val
                    elif fn == 2 and val != 0:
                        raise CheckpointError("big-endian bundles are not supported")
                continue
            e = _Entry()
            e.dtype, e.shape, e.shard, e.offset, e.size, e.crc, e.sliced = 0, (), 0, 0, 0, None, False
            for fn, _wt, val in _proto_fields(v):
                if fn == 1:
                    e.dtype = val
                elif fn == 2:
                    dims = []
                    for fn2, _w2, v2 in _proto_fields(val):
                        if fn2 == 2:
                            size = 0
                            for fn3, _w3, v3 in _proto_fields(v2):
                                if fn3 == 1:
                                    size = _signed64(v3)
                            dims.append(size)
                        elif fn2 == 3 and v2:
                            raise CheckpointError("tensor of unknown rank in the bundle")
                    e.shape = tuple(dims)
                elif fn == 3:
                    e.shard = val
                elif fn == 4:
                    e.offset = val
                elif fn == 5:
                    e.size = val
                elif fn == 6:
                    e.crc = val
                elif fn == 7:
                    e.sliced = True
            self.entries[k.decode("utf-8")] = e
        if self.num_shards is None:
            raise CheckpointError("bundle header entry is missing")
        self._shards = {}

    def keys(self):
        return sorted(self.entries)

    def __contains__(self, key):
        return key in self.entries

    def shape(self, key):
        return self.entries[key].shape

    def _shard(self, i):
        if i not in self._shards:
            path = "%s.data-%05d-of-%05d" % (self.prefix, i, self.num_shards)
            if not os.path.exists(path):
                raise FileNotFoundError(path)
            self._shards[i] = np.memmap(path, dtype=np.uint8, mode="r")
        return self._shards[i]

    def _raw(self, key):
        if key not in self.entries:
            raise KeyError("%s not in checkpoint %s" % (key, self.prefix))
        e = self.entries[key]
        if e.sliced:
            raise CheckpointError("%s: partitioned (sliced) variables are not supported" % key)
        shard = self._shard(e.shard)
        if e.offset + e.size > shard.shape[0]:
            raise CheckpointError("%s: data shard is shorter than the index says" % key)
        raw = shard[e.offset:e.offset + e.size]
        if self.verify is not False and e.crc is not None and e.dtype != DT_STRING and mask_crc(crc32c(raw)) != e.crc:
            raise CheckpointError("%s: tensor checksum mismatch" % key)
        return e, raw

    @_guard
    def get(self, key):
        e, raw = self._raw(key)
        if e.dtype == DT_STRING:
            return self._strings(key, e, bytes(raw))
        if e.dtype not in _DTYPES:
            raise CheckpointError("%s: unsupported dtype enum %d" % (key, e.dtype))
        dt = np.dtype(_DTYPES[e.dtype])
        n = int(np.prod(e.shape, dtype=np.int64)) if e.shape else 1
        if n * dt.itemsize != e.size:
            raise CheckpointError("%s: %d bytes stored for shape %s %s" % (key, e.size, e.shape, dt))
        return np.frombuffer(raw, dtype=dt).reshape(e.shape).copy()

    @staticmethod
    def _strings(key, e, raw):
        n = int(np.prod(e.shape, dtype=np.int64)) if e.shape else 1
        pos, lens = 0, []
        for _ in range(n):
            ln, pos = _varint(raw, pos)
            lens.append(ln)
        pos += 4  # masked crc32c of the lengths
        out = []
        for ln in lens:
            if pos + ln > len(raw):
                raise CheckpointError("%s: truncated string tensor" % key)
            out.append(raw[pos:pos + ln])
            pos += ln
        return out[0] if not e.shape else np.array(out, dtype=object).reshape(e.shape)


def latest_checkpoint(checkpoint_dir, latest_filename="checkpoint"):
    """``tf.train.latest_checkpoint``: the prefix named by ``model_checkpoint_path`` in <dir>/checkpoint, or None."""
    path = os.path.join(checkpoint_dir, latest_filename)
    if not os.path.exists(path):
        return None
    with open(path, "r") as f:
        m = re.search(r'^\s*model_checkpoint_path:\s*"((?:[^"\\]|\\.)*)"', f.read(), re.M)
    if not m:
        return None
    name = m.group(1).encode("utf-8").decode("unicode_escape")
    prefix = name if os.path.isabs(name) else os.path.join(checkpoint_dir, name)
    return prefix if os.path.exists(prefix + ".index") else None


# ----------------------------------------------------------------------------------------------- object graph
class ObjectGraph:
    """nodes[i] = {'children': {local_name: node_id}, 'attributes': [(name, full_name, checkpoint_key)]}"""

    @_guard
    def __init__(self, blob):
        self.nodes = []
        for fn, _wt, val in _proto_fields(blob):
            if fn != 1:
                continue
            node = {"children": {}, "attributes": []}
            for fn2, _w2, v2 in _proto_fields(val):
                if fn2 == 1:
                    nid, lname = 0, ""
                    for fn3, _w3, v3 in _proto_fields(v2):
                        if fn3 == 1:
                            nid = v3
                        elif fn3 == 2:
                            lname = v3.decode("utf-8")
                    node["children"][lname] = nid
                elif fn2 == 2:
                    name = full = ckey = ""
                    for fn3, _w3, v3 in _proto_fields(v2):
                        if fn3 == 1:
                            name = v3.decode("utf-8")
                        elif fn3 == 2:
                            full = v3.decode("utf-8")
                        elif fn3 == 3:
                            ckey = v3.decode("utf-8")
                    node["attributes"].append((name, full, ckey))
            self.nodes.append(node)
        if not self.nodes:
            raise CheckpointError("empty object graph")

    def child(self, node_id, name):
        return self.nodes[node_id]["children"].get(name)

    def variable(self, node_id):
        """(full_name, checkpoint_key) of a variable node, or None"""
        for name, full, ckey in self.nodes[node_id]["attributes"]:
            if name == "VARIABLE_VALUE":
                return full, ckey
        return None


# ----------------------------------------------------------------------------------------------- the reference's checkpoint -> Keras-layout dict
def keras_weighted_layer_order(shortcut_first=False):
    """Names of the ResNet50 layers that own weights in ``model.layers`` order = the ``layer_with_weights-N`` numbering.
    keras_applications 1.0.8 (TF 2.0, the reference's pin): ... 2c conv, shortcut conv, 2c bn, shortcut bn (the shortcut is
    the *second* input of the add); tf.keras >= 2.2 builds the shortcut first: shortcut conv, 2c conv, shortcut bn, 2c bn."""
    names = ["conv1", "bn_conv1"]
    by_block = {}
    for s in CONV_SPECS[1:]:
        by_block.setdefault(s.name.split("_branch")[0], []).append(s)
    for blk in by_block.values():
        d = {s.name.split("_branch")[1]: s for s in blk}
        names += [d["2a"].name, d["2a"].bn_name, d["2b"].name, d["2b"].bn_name]
        tail = [d["2c"]] + ([d["1"]] if "1" in d else [])
        if shortcut_first:
            tail.reverse()
        names += [s.name for s in tail] + [s.bn_name for s in tail]
    return names


_BN_VARS = ("gamma", "beta", "moving_mean", "moving_variance")
# tf.keras >= 2.2 layer names -> the keras_applications 1.0.8 names the C ABI uses (resnet_spec.CONV_SPECS)


def _modern_to_legacy(layer):
    if layer == "conv1_conv":
        return "conv1"
    if layer == "conv1_bn":
        return "bn_conv1"
    m = re.fullmatch(r"conv([2-5])_block(\d)_([0-3])_(conv|bn)", layer)
    if not m:
        return None
    stage, blk, idx, kind = int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4)
    branch = {0: "1", 1: "2a", 2: "2b", 3: "2c"}[idx]
    return "%s%d%s_branch%s" % ("res" if kind == "conv" else "bn", stage, "abcdef"[blk - 1], branch)


def _shape_ok(name, arr_shape):
    for s in CONV_SPECS:
        if s.name == name:
            return tuple(arr_shape) == (s.kh, s.kw, s.cin, s.cout)
    return True


def load_hmr_weights(prefix_or_dir, verify=True):
    """-> (weights, info).  ``weights`` is the Keras-layout dict ``HpeEngine.load_encoder`` / ``load_regressor`` take
    (``<layer>/kernel`` HWIO, ``<layer>/bias``, ``<bn>/gamma|beta|moving_mean|moving_variance``, ``dense_{0,1,2}/kernel|bias``)
    plus ``inital_theta`` [1,85] when the checkpoint has it (src/predictor.py:84 -- the attribute name is misspelt in the
    reference and therefore in its checkpoints).  ``info`` says how names were resolved."""
    prefix = str(prefix_or_dir)
    if os.path.isdir(prefix):
        p = latest_checkpoint(prefix)
        if p is None:
            raise FileNotFoundError("no TensorFlow checkpoint state in %s" % prefix)
        prefix = p
    rd = BundleReader(prefix, verify=verify)
    out, info = {}, {"prefix": prefix, "resolved_by": None}
    known = {s.name for s in CONV_SPECS} | {s.bn_name for s in CONV_SPECS}

    def put_layer(layer, var, ckey):
        out["%s/%s" % (layer, var)] = rd.get(ckey)

    graph = ObjectGraph(rd.get(OBJECT_GRAPH_KEY)) if OBJECT_GRAPH_KEY in rd else None
    enc_done = False
    if graph is not None:
        fe = graph.child(0, "feature_extractor")
        if fe is not None:
            for lname, nid in graph.nodes[fe]["children"].items():
                if not lname.startswith("layer_with_weights-"):
                    continue
                for var, vid in graph.nodes[nid]["children"].items():
                    v = graph.variable(vid)
                    if v is None:
                        continue
                    full, ckey = v
                    layer = full.split("/")[-2] if "/" in full else ""
                    layer = layer if layer in known else (_modern_to_legacy(layer) or layer)
                    if layer in known and ckey in rd:
                        put_layer(layer, var, ckey)
            enc_done = all(("%s/kernel" % s.name) in out and ("%s/gamma" % s.bn_name) in out for s in CONV_SPECS)
            if enc_done:
                info["resolved_by"] = "object graph (Keras variable names)"
    if not enc_done:
        # positional: feature_extractor/layer_with_weights-N in model.layers order; decide the order of the two equal-depth
        # 1x1 convs at a block end from a block where their shapes differ (res3a: shortcut [1,1,256,512] vs 2c [1,1,128,512])
        base = "feature_extractor/layer_with_weights-%d/%s" + VAR_SUFFIX
        for shortcut_first in (False, True):
            order = keras_weighted_layer_order(shortcut_first)
            i3 = order.index("res3a_branch1")
            k = base % (i3, "kernel")
            if k in rd and rd.shape(k) == (1, 1, 256, 512):
                break
        else:
            raise CheckpointError("feature_extractor weights not found in %s (neither by name nor by position)" % prefix)
        for i, layer in enumerate(order):
            for var in (("kernel", "bias") if not layer.startswith("bn") else _BN_VARS):
                put_layer(layer, var, base % (i, var))
        info["resolved_by"] = "position (%s order)" % ("tf.keras>=2.2" if shortcut_first else "keras_applications 1.0.8")
    for s in CONV_SPECS:
        if not _shape_ok(s.name, out[s.name + "/kernel"].shape):
            raise CheckpointError("%s/kernel has shape %s, expected %s" % (s.name, out[s.name + "/kernel"].shape, (s.kh, s.kw, s.cin, s.cout)))
    # regressor: a Sequential -- its three Dense layers are layer_with_weights-0..2 whatever their auto-generated names
    for i, name in enumerate(("dense_0", "dense_1", "dense_2")):
        for var in ("kernel", "bias"):
            ckey = "generator3d/layer_with_weights-%d/%s%s" % (i, var, VAR_SUFFIX)
            if graph is not None:
                g3 = graph.child(0, "generator3d")
                nid = graph.child(g3, "layer_with_weights-%d" % i) if g3 is not None else None
                vid = graph.child(nid, var) if nid is not None else None
                v = graph.variable(vid) if vid is not None else None
                if v is not None:
                    ckey = v[1]
            out["%s/%s" % (name, var)] = rd.get(ckey)
    ckey = "inital_theta" + VAR_SUFFIX
    if ckey in rd:
        out["inital_theta"] = rd.get(ckey)
    # the trained mean theta: a root only ``save_checkpoint`` writes (the reference's checkpoints do not hold it, see the writer)
    ckey = "mean_var" + VAR_SUFFIX
    if ckey in rd:
        out["mean_var"] = rd.get(ckey)
    return out, info


# ----------------------------------------------------------------------------------------------- the checkpoint's critic
# CriticNetwork's Dense layers (src/models.py:158-202): Keras layer name -> kernel shape [in, out]; all nine shapes differ
CRITIC_SHAPES = {name: (fi, fo) for name, fi, fo in CRITIC_LAYERS}


class NoCriticError(CheckpointError):
    """the checkpoint holds no discriminator at all (one that is present but incomplete or misshapen is a plain CheckpointError)"""


def load_critic_weights(prefix_or_dir, verify=True):
    """-> (weights, info): the checkpoint's ``discriminator`` (the CriticNetwork, src/trainer.py:193-198) as the dict
    ``HpeEngine.load_critic`` takes: ``critic/<Keras layer name>/kernel`` [in,out] and ``critic/<Keras layer name>/bias`` [out].
    Layers are found by their Keras names through the object graph; failing that (no graph, or names that say nothing) each
    ``discriminator/layer_with_weights-N`` is assigned by its kernel shape, which is unambiguous because all nine differ.  Every
    shape is verified either way.  A checkpoint without any discriminator raises NoCriticError (with an object graph: no
    ``discriminator`` child of the root -- what a restore would see; without one: no ``discriminator/layer_with_weights-N`` key); one
    that is there but incomplete or misshapen raises CheckpointError."""
    prefix = str(prefix_or_dir)
    if os.path.isdir(prefix):
        p = latest_checkpoint(prefix)
        if p is None:
            raise FileNotFoundError("no TensorFlow checkpoint state in %s" % prefix)
        prefix = p
    rd = BundleReader(prefix, verify=verify)
    info = {"prefix": prefix, "resolved_by": None}
    keys = {}  # Keras layer name -> {"kernel": checkpoint key, "bias": checkpoint key}
    slots = {}  # N of layer_with_weights-N -> {"kernel": checkpoint key, "bias": checkpoint key}
    graph = ObjectGraph(rd.get(OBJECT_GRAPH_KEY)) if OBJECT_GRAPH_KEY in rd else None
    disc = graph.child(0, "discriminator") if graph is not None else None
    if disc is not None:
        for lname, nid in graph.nodes[disc]["children"].items():
            m = re.fullmatch(r"layer_with_weights-(\d+)", lname)
            if not m:
                continue
            for var, vid in graph.nodes[nid]["children"].items():
                v = graph.variable(vid)
                if v is None or var not in ("kernel", "bias") or v[1] not in rd:
                    continue
                full, ckey = v
                slots.setdefault(int(m.group(1)), {})[var] = ckey
                layer = full.split("/")[-2] if "/" in full else ""
                if layer in CRITIC_SHAPES:
                    keys.setdefault(layer, {})[var] = ckey
    elif graph is not None:
        raise NoCriticError("%s has no discriminator (critic): its object graph has no such child" % prefix)
    else:
        for k in rd.keys():
            m = re.fullmatch(r"discriminator/layer_with_weights-(\d+)/(kernel|bias)" + re.escape(VAR_SUFFIX), k)
            if m:
                slots.setdefault(int(m.group(1)), {})[m.group(2)] = k
    complete = lambda d: len(d) == len(CRITIC_SHAPES) and all(len(v) == 2 for v in d.values())  # noqa: E731
    if complete(keys):
        info["resolved_by"] = "object graph (Keras variable names)"
    else:
        by_shape = {shape: name for name, shape in CRITIC_SHAPES.items()}
        keys = {}
        for n in sorted(slots):
            ck = slots[n]
            name = by_shape.get(tuple(rd.shape(ck["kernel"]))) if "kernel" in ck else None
            if name is not None and name not in keys and "bias" in ck:
                keys[name] = ck
        if not complete(keys):
            if not slots:
                raise NoCriticError("%s has no discriminator (critic): no discriminator/layer_with_weights-N variables" % prefix)
            missing = sorted(set(CRITIC_SHAPES) - set(keys))
            raise CheckpointError("%s: the discriminator (critic) is incomplete: missing %s" % (prefix, ", ".join(missing)))
        info["resolved_by"] = "kernel shape"
    out = {}
    for name, (fi, fo) in CRITIC_SHAPES.items():
        k, b = rd.get(keys[name]["kernel"]), rd.get(keys[name]["bias"])
        if k.shape != (fi, fo) or b.shape != (fo,):
            raise CheckpointError("critic layer %s has kernel %s and bias %s, expected %s and %s" % (name, k.shape, b.shape, (fi, fo), (fo,)))
        out["critic/%s/kernel" % name], out["critic/%s/bias" % name] = k, b
    return out, info


# =============================================================================================== the writer
# ``save_checkpoint`` writes the layout described at the top of this file: what ``tf.train.Checkpoint.save`` of the reference's Trainer
# (src/trainer.py:193-198, 836) leaves on disk, so that a model trained here can be restored by ``Predictor(config)``, resumed by
# ``load_training_state``, and is laid out for the reference's own ``checkpoint.restore``.  Written from the published format
# descriptions (LevelDB table_format.md; tensor_bundle.proto; trackable_object_graph.proto; checkpoint_state.proto), sharing only the
# CRC and the constants with the reader above.
#
# PARITY UNPINNED, as for the reader: no TensorFlow exists in this environment, so no file written here has been restored by
# TensorFlow and none written by TensorFlow has been compared with one written here.  Tested: the reader above and the independent
# test writer (tests/tf_bundle_writer.py) agree with it.
#
# One root is this project's own: ``mean_var``.  The reference trains ``mean_var`` (src/trainer.py:482) but tracks only the untrained
# ``theta_prev`` as ``inital_theta``, so its checkpoints lose the trained mean; here the trained mean theta is saved as ``mean_var``
# (with its optimiser slots) and ``inital_theta`` keeps the reference's meaning.  A restore that does not know the extra root skips it.
OPTIMIZER_ROOTS = ("generator_optimizer", "discriminator_optimizer")
_HYPER = ("learning_rate", "beta_1", "beta_2", "decay")
_NP_TO_DT = {"float32": 1, "float64": 2, "int32": 3, "int64": 9}
_BLOCK_BYTES = 4096
_RESTART_INTERVAL = 16


def _enc_varint(n):
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


def _pb_varint(fn, v):
    return _enc_varint(fn << 3) + _enc_varint(v)


def _pb_bytes(fn, payload):
    return _enc_varint((fn << 3) | 2) + _enc_varint(len(payload)) + payload


def _pb_str(fn, s):
    return _pb_bytes(fn, s.encode("utf-8"))


def _pb_fixed32(fn, v):
    return _enc_varint((fn << 3) | 5) + int(v).to_bytes(4, "little")


class _BlockWriter:
    """one table block: entries (shared, non_shared, value_length, key suffix, value) with a restart point every `interval` entries, then
    the restart offsets and their count as fixed32"""

    def __init__(self, interval):
        self.interval, self.buf, self.restarts, self.count, self.last = interval, bytearray(), [], 0, b""

    def add(self, key, value):
        shared = 0
        if self.count % self.interval == 0:
            self.restarts.append(len(self.buf))
        else:
            limit = min(len(key), len(self.last))
            while shared < limit and key[shared] == self.last[shared]:
                shared += 1
        self.buf += _enc_varint(shared) + _enc_varint(len(key) - shared) + _enc_varint(len(value)) + key[shared:] + value
        self.last = key
        self.count += 1

    def finish(self):
        restarts = self.restarts or [0]
        return bytes(self.buf) + b"".join(r.to_bytes(4, "little") for r in restarts) + len(restarts).to_bytes(4, "little")


def _write_table(path, items):
    """items: [(key bytes, value bytes)] in ascending key order -> a LevelDB-format table without compression or filter"""
    out = bytearray()

    def emit(block):
        handle = _enc_varint(len(out)) + _enc_varint(len(block))
        out.extend(block)
        out.append(0)  # kNoCompression
        out.extend(mask_crc(crc32c(block + b"\0")).to_bytes(4, "little"))
        return handle

    index = _BlockWriter(1)
    cur = _BlockWriter(_RESTART_INTERVAL)
    prev = None
    for key, value in items:
        if prev is not None and key <= prev:
            raise CheckpointError("table keys must be strictly ascending")
        cur.add(key, value)
        prev = key
        if len(cur.buf) >= _BLOCK_BYTES:
            index.add(key, emit(cur.finish()))  # the block's last key separates it from the next
            cur = _BlockWriter(_RESTART_INTERVAL)
    if cur.count:
        index.add(prev, emit(cur.finish()))
    meta = emit(_BlockWriter(1).finish())
    idx = emit(index.finish())
    footer = meta + idx
    out.extend(footer + b"\0" * (40 - len(footer)) + TABLE_MAGIC.to_bytes(8, "little"))
    with open(path, "wb") as f:
        f.write(out)


def _string_tensor_bytes(s):
    """a scalar DT_STRING tensor in a data shard: the length as a varint, the masked CRC of the lengths (as uint32 each), the bytes; the
    entry's own checksum runs over the lengths, that checksum and the bytes"""
    crc = crc32c(len(s).to_bytes(4, "little"))
    check = mask_crc(crc).to_bytes(4, "little")
    return _enc_varint(len(s)) + check + s, crc32c(s, crc32c(check, crc))


def write_bundle(prefix, tensors):
    """tensors: {checkpoint key: ndarray (float32 / float64 / int32 / int64) or bytes (a scalar string tensor)} -> ``prefix.index`` and
    ``prefix.data-00000-of-00001``"""
    header = _pb_varint(1, 1) + _pb_bytes(3, _pb_varint(1, 1))  # num_shards = 1, little endian (the default), version.producer = 1
    items = [(b"", header)]
    offset = 0
    with open(prefix + ".data-00000-of-00001", "wb") as data:
        for key in sorted(tensors, key=lambda k: k.encode("utf-8")):
            t = tensors[key]
            if isinstance(t, (bytes, bytearray)):
                payload, crc = _string_tensor_bytes(bytes(t))
                entry = _pb_varint(1, DT_STRING) + _pb_bytes(2, b"")
            else:
                t = np.asarray(t)
                t = t if t.flags.c_contiguous else np.ascontiguousarray(t)  # (ascontiguousarray alone would make a scalar [1])
                if t.dtype.name not in _NP_TO_DT:
                    raise CheckpointError("%s: dtype %s cannot be written" % (key, t.dtype))
                t = t.astype(t.dtype.newbyteorder("<"), copy=False)
                payload = t.tobytes()
                crc = crc32c(t) if t.size else crc32c(b"")
                shape = b"".join(_pb_bytes(2, _pb_varint(1, d)) for d in t.shape)
                entry = _pb_varint(1, _NP_TO_DT[t.dtype.name]) + _pb_bytes(2, shape)
            if offset:
                entry += _pb_varint(4, offset)
            entry += _pb_varint(5, len(payload)) + _pb_fixed32(6, mask_crc(crc))
            data.write(payload)
            offset += len(payload)
            items.append((key.encode("utf-8"), entry))
    _write_table(prefix + ".index", items)


class _GraphBuilder:
    """TrackableObjectGraph: nodes numbered breadth-first from the root, slot variables after them"""

    def __init__(self):
        self.children = [[]]  # per node [(local name, node id)]
        self.attrs = [None]  # per node (full_name, checkpoint_key) or None
        self.slots = [[]]  # per node [(original node id, slot name, slot node id)]

    def _new(self):
        self.children.append([])
        self.attrs.append(None)
        self.slots.append([])
        return len(self.children) - 1

    def child(self, parent, name):
        nid = self._new()
        self.children[parent].append((name, nid))
        return nid

    def variable(self, parent, name, full_name, key):
        nid = self.child(parent, name)
        self.attrs[nid] = (full_name, key)
        return nid

    def slot(self, optimizer, original, slot_name, full_name, key):
        nid = self._new()
        self.attrs[nid] = (full_name, key)
        self.slots[optimizer].append((original, slot_name, nid))
        return nid

    def serialize(self):
        out = b""
        for ch, at, sl in zip(self.children, self.attrs, self.slots):
            body = b"".join(_pb_bytes(1, _pb_varint(1, nid) + _pb_str(2, name)) for name, nid in ch)
            if at is not None:
                body += _pb_bytes(2, _pb_str(1, "VARIABLE_VALUE") + _pb_str(2, at[0]) + _pb_str(3, at[1]))
            body += b"".join(_pb_bytes(3, _pb_varint(1, o) + _pb_str(2, n) + _pb_varint(3, s)) for o, n, s in sl)
            out += _pb_bytes(1, body)
        return out


def _keras_dense_name(i):
    return "dense" if i == 0 else "dense_%d" % i


def _model_variables():
    """[(root, object path under the root, Keras full_name, project key)] of every variable of the three networks, in the order the
    object graph lists them"""
    out = []
    bn_of = {s.bn_name for s in CONV_SPECS}
    for i, layer in enumerate(keras_weighted_layer_order(False)):
        for var in (_BN_VARS if layer in bn_of else ("kernel", "bias")):
            out.append(("feature_extractor", "layer_with_weights-%d/%s" % (i, var), "%s/%s" % (layer, var), "%s/%s" % (layer, var)))
    for i in range(3):
        for var in ("kernel", "bias"):
            out.append(("generator3d", "layer_with_weights-%d/%s" % (i, var), "%s/%s" % (_keras_dense_name(i), var), "dense_%d/%s" % (i, var)))
    for i, (name, _fi, _fo) in enumerate(CRITIC_LAYERS):
        for var in ("kernel", "bias"):
            out.append(("discriminator", "layer_with_weights-%d/%s" % (i, var), "%s/%s" % (name, var), "critic/%s/%s" % (name, var)))
    return out


def _read_state_paths(checkpoint_dir):
    path = os.path.join(checkpoint_dir, "checkpoint")
    if not os.path.exists(path):
        return []
    with open(path, "r") as f:
        return re.findall(r'^\s*all_model_checkpoint_paths:\s*"((?:[^"\\]|\\.)*)"', f.read(), re.M)


def write_checkpoint_state(checkpoint_dir, name):
    """the ``checkpoint`` state file (CheckpointState in text format): ``name`` becomes the newest, earlier ones stay listed"""
    older = [p for p in _read_state_paths(checkpoint_dir) if p != name]
    tmp = os.path.join(checkpoint_dir, "checkpoint.tmp%d" % os.getpid())
    with open(tmp, "w") as f:
        f.write('model_checkpoint_path: "%s"\n' % name)
        for p in older + [name]:
            f.write('all_model_checkpoint_paths: "%s"\n' % p)
    os.replace(tmp, os.path.join(checkpoint_dir, "checkpoint"))


def save_checkpoint(prefix, weights, inital_theta=None, mean_var=None, optimizers=None, save_counter=1, update_state=True):
    """Write ``prefix.index`` / ``prefix.data-00000-of-00001`` (``prefix`` = ``<dir>/ckpt-N``) and, with ``update_state``, name it in
    ``<dir>/checkpoint``.

    weights: the Keras-layout dict of ``load_encoder`` + ``load_regressor`` (+ ``load_critic``'s ``critic/...`` keys; without them the
    checkpoint has no ``discriminator``).  inital_theta [1,85]: the reference's untrained ``theta_prev``; mean_var [85] or [1,85]: the
    trained mean theta (see above).  optimizers: {"generator_optimizer" | "discriminator_optimizer": {"iterations", "learning_rate",
    "beta_1", "beta_2", "decay" (default 0), "slots": {project key: {"m": array, "v": array}}}} where a project key is a key of
    ``weights`` or "mean_var" (``flat_slots`` splits a flat optimiser tensor into them); a variable without slots simply has none.
    -> prefix"""
    prefix = str(prefix)
    g = _GraphBuilder()
    tensors = {}
    opt_nodes = {}
    # breadth-first: the root's children first, in the reference's constructor order
    roots = {}
    for name in OPTIMIZER_ROOTS:
        if optimizers and name in optimizers:
            roots[name] = opt_nodes[name] = g.child(0, name)
    has_critic = any(k.startswith("critic/") for k in weights)
    for name in ("feature_extractor", "generator3d") + (("discriminator",) if has_critic else ()):
        roots[name] = g.child(0, name)
    var_nodes = {}  # project key -> (node id, object path)

    def put(parent, local, full, path, value, dtype, key=None):
        ckey = path + VAR_SUFFIX
        nid = g.variable(parent, local, full, ckey)
        tensors[ckey] = np.asarray(value, dtype)
        if key is not None:
            var_nodes[key] = (nid, path)

    if inital_theta is not None:
        put(0, "inital_theta", "mean_param", "inital_theta", np.asarray(inital_theta, np.float32).reshape(1, 85), np.float32)
    if mean_var is not None:
        put(0, "mean_var", "mean_param_1", "mean_var", np.asarray(mean_var, np.float32).reshape(1, 85), np.float32, key="mean_var")
    put(0, "save_counter", "save_counter", "save_counter", int(save_counter), np.int64)
    for name, node in opt_nodes.items():
        o = optimizers[name]
        put(node, "iter", "Adam/iter", name + "/iter", int(o["iterations"]), np.int64)
        for h in _HYPER:
            put(node, h, "Adam/" + h, "%s/%s" % (name, h), float(o.get(h, 0.0)), np.float32)
    layers = {}
    model_vars = [mv for mv in _model_variables() if mv[0] in roots]
    for root, path, _full, _key in model_vars:  # the layer objects of each network ...
        lname = path.split("/")[0]
        if (root, lname) not in layers:
            layers[root, lname] = g.child(roots[root], lname)
    for root, path, full, key in model_vars:  # ... then their variables
        if key not in weights:
            raise KeyError("weights has no %s" % key)
        lname, var = path.split("/")
        put(layers[root, lname], var, full, "%s/%s" % (root, path), weights[key], np.float32, key=key)
    for name, node in opt_nodes.items():
        for key, mv in optimizers[name].get("slots", {}).items():
            if key not in var_nodes:
                raise KeyError("optimiser slots for %s, which is not a saved variable" % key)
            nid, path = var_nodes[key]
            shape = tensors[path + VAR_SUFFIX].shape
            for s in ("m", "v"):
                ckey = "%s/.OPTIMIZER_SLOT/%s/%s%s" % (path, name, s, VAR_SUFFIX)
                a = np.asarray(mv[s], np.float32)
                if a.size != int(np.prod(shape, dtype=np.int64)):
                    raise ValueError("slot %s of %s holds %d values, the variable %s" % (s, key, a.size, shape))
                tensors[ckey] = a.reshape(shape)
                g.slot(node, nid, s, "Adam/%s/%s" % (g.attrs[nid][0], s), ckey)
    tensors[OBJECT_GRAPH_KEY] = g.serialize()
    os.makedirs(os.path.dirname(prefix) or ".", exist_ok=True)
    write_bundle(prefix, tensors)
    if update_state:
        write_checkpoint_state(os.path.dirname(prefix) or ".", os.path.basename(prefix))
    return prefix


def _flat_tables():
    """{"encoder" | "regressor" | "critic": ([(project key, offset, size)], total floats)} of the three flat layouts"""
    from . import critic_spec, regressor_spec, resnet_spec

    enc = []
    for s, off in zip(CONV_SPECS, resnet_spec.ENCODER_PARAM_OFFSETS):
        sizes = (s.kh * s.kw * s.cin * s.cout, s.cout, s.cout, s.cout)
        enc += [(k, o, n) for k, o, n in zip(resnet_spec._flat_keys(s), off, sizes)]
    reg = [("mean_var" if k == "mean_theta" else k, o, int(np.prod(shp))) for k, o, shp in regressor_spec.flat_layout()]
    cri = [(k, o, int(np.prod(shp))) for k, o, shp in critic_spec.flat_layout()]
    return {"encoder": (enc, resnet_spec.ENCODER_PARAM_FLOATS), "regressor": (reg, regressor_spec.PARAM_FLOATS), "critic": (cri, critic_spec.PARAM_FLOATS)}


def flat_slots(layout, m, v):
    """the moments of one flat optimiser tensor (``layout``: "encoder" = resnet_spec, "regressor" = regressor_spec with mean theta as
    "mean_var", "critic" = critic_spec) -> {project key: {"m", "v"}} as ``save_checkpoint`` takes them"""
    table, total = _flat_tables()[layout]
    m, v = (np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float32).reshape(-1) for a in (m, v))
    if m.size != total or v.size != total:
        raise ValueError("%s moments must hold %d floats" % (layout, total))
    return {k: {"m": m[o:o + n], "v": v[o:o + n]} for k, o, n in table}


def _graph_slots(blob):
    """[(optimizer node id, original node id, slot name, slot node id)]: the slot_variables records of every node"""
    out = []
    node = 0
    for fn, _wt, val in _proto_fields(blob):
        if fn != 1:
            continue
        for fn2, _w2, v2 in _proto_fields(val):
            if fn2 == 3:
                rec = {1: 0, 2: b"", 3: 0}
                for fn3, _w3, v3 in _proto_fields(v2):
                    rec[fn3] = v3
                out.append((node, rec[1], rec[2].decode("utf-8"), rec[3]))
        node += 1
    return out


@_guard
def load_training_state(prefix_or_dir, verify=True):
    """What a resumed run needs besides the weights: per optimiser of the reference's checkpoint its ``iter``, its hyper-parameters and
    its moments, mapped back to the flat layouts.  ->
    {"prefix", "save_counter", "mean_var" ([85] or None),
     "generator_optimizer": {"iter", "learning_rate", "beta_1", "beta_2", "decay", "slots": {project key: {"m", "v"}},
                             "encoder": {"m", "v"} (flat, resnet_spec) or None, "regressor": {"m", "v"} (flat, regressor_spec) or None,
                             "missing": [project keys of those layouts without slots: zeros in the flat tensors]},
     "discriminator_optimizer": {..., "critic": {"m", "v"} (flat, critic_spec) or None, "missing": [...]}}
    A checkpoint with weights but no optimiser state (a weights-only export; the reference restores such a file with
    ``expect_partial()`` and starts fresh moments) raises CheckpointError: the caller decides to start fresh."""
    prefix = str(prefix_or_dir)
    if os.path.isdir(prefix):
        p = latest_checkpoint(prefix)
        if p is None:
            raise FileNotFoundError("no TensorFlow checkpoint state in %s" % prefix)
        prefix = p
    rd = BundleReader(prefix, verify=verify)
    if OBJECT_GRAPH_KEY not in rd:
        raise CheckpointError("%s has no optimiser state (no object graph)" % prefix)
    blob = rd.get(OBJECT_GRAPH_KEY)
    graph = ObjectGraph(blob)
    records = _graph_slots(blob)
    opt_ids = {name: graph.child(0, name) for name in OPTIMIZER_ROOTS}
    if all(v is None for v in opt_ids.values()) or not records:
        raise CheckpointError("%s has weights but no optimiser state (no generator_optimizer / discriminator_optimizer slots): "
                              "start fresh moments" % prefix)
    # node id -> project key, through the Keras names as load_hmr_weights / load_critic_weights resolve them
    key_of = {}
    known = {s.name for s in CONV_SPECS} | {s.bn_name for s in CONV_SPECS}

    def layer_vars(root):
        rid = graph.child(0, root)
        if rid is None:
            return
        for lname, nid in graph.nodes[rid]["children"].items():
            m = re.fullmatch(r"layer_with_weights-(\d+)", lname)
            if m:
                for var, vid in graph.nodes[nid]["children"].items():
                    v = graph.variable(vid)
                    if v is not None:
                        yield int(m.group(1)), var, vid, v[0], v[1]

    for _i, var, vid, full, _ck in layer_vars("feature_extractor"):
        layer = full.split("/")[-2] if "/" in full else ""
        layer = layer if layer in known else (_modern_to_legacy(layer) or layer)
        if layer in known:
            key_of[vid] = "%s/%s" % (layer, var)
    for i, var, vid, _full, _ck in layer_vars("generator3d"):
        if i < 3 and var in ("kernel", "bias"):
            key_of[vid] = "dense_%d/%s" % (i, var)
    by_shape = {shape: name for name, shape in CRITIC_SHAPES.items()}
    crit = {}
    for i, var, vid, full, ck in layer_vars("discriminator"):
        crit.setdefault(i, {})[var] = (vid, full, ck)
    for i, d in crit.items():
        layer = d["kernel"][1].split("/")[-2] if "kernel" in d and "/" in d["kernel"][1] else ""
        if layer not in CRITIC_SHAPES and "kernel" in d and d["kernel"][2] in rd:
            layer = by_shape.get(tuple(rd.shape(d["kernel"][2])), "")
        if layer in CRITIC_SHAPES:
            for var, (vid, _f, _c) in d.items():
                key_of[vid] = "critic/%s/%s" % (layer, var)
    mv = graph.child(0, "mean_var")
    if mv is not None:
        key_of[mv] = "mean_var"
    out = {"prefix": prefix, "save_counter": None, "mean_var": None}
    sc = graph.child(0, "save_counter")
    if sc is not None and graph.variable(sc) is not None:
        out["save_counter"] = int(rd.get(graph.variable(sc)[1]).reshape(-1)[0])
    if mv is not None and graph.variable(mv) is not None:
        out["mean_var"] = rd.get(graph.variable(mv)[1]).reshape(-1)
    tables = _flat_tables()
    for name, oid in opt_ids.items():
        if oid is None:
            continue
        st = {"slots": {}, "missing": []}
        for h in ("iter",) + _HYPER:
            hid = graph.child(oid, h)
            v = graph.variable(hid) if hid is not None else None
            val = rd.get(v[1]) if v is not None else None
            st[h] = None if val is None else (int(val.reshape(-1)[0]) if h == "iter" else float(val.reshape(-1)[0]))
        if st["iter"] is None:
            raise CheckpointError("%s: %s has no iter" % (prefix, name))
        for onode, orig, sname, sid in records:
            if onode != oid or orig not in key_of or sname not in ("m", "v"):
                continue
            v = graph.variable(sid) if 0 <= sid < len(graph.nodes) else None
            if v is None:
                raise CheckpointError("%s: slot variable node %d of %s holds no value" % (prefix, sid, name))
            st["slots"].setdefault(key_of[orig], {})[sname] = rd.get(v[1])
        for key, mvs in st["slots"].items():
            if set(mvs) != {"m", "v"}:
                raise CheckpointError("%s: %s has only one of the slots m and v for %s" % (prefix, name, key))
        for layout in (("encoder", "regressor") if name == "generator_optimizer" else ("critic",)):
            table, total = tables[layout]
            if not any(k in st["slots"] for k, _o, _n in table):
                st[layout] = None
                continue
            flat = {"m": np.zeros(total, np.float32), "v": np.zeros(total, np.float32)}
            for k, o, n in table:
                if k not in st["slots"]:
                    st["missing"].append(k)
                    continue
                for s in ("m", "v"):
                    a = st["slots"][k][s]
                    if a.size != n:
                        raise CheckpointError("%s: slot %s of %s holds %d values, expected %d" % (prefix, s, k, a.size, n))
                    flat[s][o:o + n] = a.reshape(-1)
            st[layout] = flat
        out[name] = st
    if not any(out.get(n, {}).get("slots") for n in OPTIMIZER_ROOTS):
        raise CheckpointError("%s has weights but no optimiser state (its optimisers hold no slots): start fresh moments" % prefix)
    return out
