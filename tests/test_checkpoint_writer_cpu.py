"""The checkpoint writer (tf_checkpoint.save_checkpoint) against the package's reader, and ``load_training_state``.  PARITY UNPINNED: no
TensorFlow exists here; what is pinned is that writer and reader, written separately from the same format descriptions, agree, and that
the independent test writer (tests/tf_bundle_writer.py) and the package's produce bundles the same reader accepts."""
import os

import numpy as np
import pytest

import tf_bundle_writer as W
from hpe_amd import critic_spec, regressor_spec, resnet_spec, synthetic, tf_checkpoint as T
from hpe_amd.resnet_spec import CONV_SPECS

SUF = T.VAR_SUFFIX
# optimiser slots for a reduced set of variables: one layer of each kind (the 7x7 stem, a 1x1, a 3x3 and a shortcut convolution with
# their BatchNorm scale and offset; a Dense layer of the regressor; the trained mean theta; two Dense layers of the critic)
GEN_SLOT_KEYS = ("conv1/kernel", "conv1/bias", "bn_conv1/gamma", "bn_conv1/beta", "res2a_branch2a/kernel", "res2a_branch2b/kernel",
                 "bn2a_branch2b/gamma", "res2a_branch1/kernel", "bn2a_branch1/beta", "dense_2/kernel", "dense_2/bias", "mean_var")
CRITIC_SLOT_KEYS = ("critic/kcs_dense/kernel", "critic/kcs_dense/bias", "critic/shapes_dense_3/kernel", "critic/shapes_dense_3/bias")


@pytest.fixture(scope="module")
def weights():
    w = dict(synthetic.make_encoder_params(seed=1))
    w.update(synthetic.make_regressor_params(seed=2))
    rng = np.random.default_rng(3)
    for key, _off, shape in critic_spec.flat_layout():
        w[key] = rng.normal(size=shape).astype(np.float32)
    return w


def _slots(weights, keys, seed):
    rng = np.random.default_rng(seed)
    shape = lambda k: (85,) if k == "mean_var" else weights[k].shape  # noqa: E731
    return {k: {"m": rng.normal(size=shape(k)).astype(np.float32), "v": (rng.normal(size=shape(k)) ** 2).astype(np.float32)} for k in keys}


def _optimizers(weights):
    return {"generator_optimizer": {"iterations": 2 ** 33 + 5, "learning_rate": 1e-4, "beta_1": 0.9, "beta_2": 0.999,
                                    "slots": _slots(weights, GEN_SLOT_KEYS, 10)},
            "discriminator_optimizer": {"iterations": 7, "learning_rate": 5e-4, "beta_1": 0.9, "beta_2": 0.999, "decay": 0.0,
                                        "slots": _slots(weights, CRITIC_SLOT_KEYS, 11)}}


def _assert_weights(w, weights):
    for s in CONV_SPECS:
        for var in ("kernel", "bias"):
            np.testing.assert_array_equal(w["%s/%s" % (s.name, var)], weights["%s/%s" % (s.name, var)])
        for var in T._BN_VARS:
            np.testing.assert_array_equal(w["%s/%s" % (s.bn_name, var)], weights["%s/%s" % (s.bn_name, var)])
    for i in range(3):
        for var in ("kernel", "bias"):
            np.testing.assert_array_equal(w["dense_%d/%s" % (i, var)], weights["dense_%d/%s" % (i, var)])


@pytest.fixture(scope="module")
def saved(tmp_path_factory, weights):
    d = tmp_path_factory.mktemp("ckpt")
    theta0 = np.random.default_rng(4).normal(size=(1, 85)).astype(np.float32)
    mean = np.random.default_rng(5).normal(size=85).astype(np.float32)
    opts = _optimizers(weights)
    prefix = T.save_checkpoint(str(d / "ckpt-1"), weights, inital_theta=theta0, mean_var=mean, optimizers=opts, save_counter=1)
    return str(d), prefix, theta0, mean, opts


def test_full_size_weights_round_trip(saved, weights):
    d, prefix, theta0, mean, _opts = saved
    assert prefix == os.path.join(d, "ckpt-1") and T.latest_checkpoint(d) == prefix
    assert sorted(os.listdir(d)) == ["checkpoint", "ckpt-1.data-00000-of-00001", "ckpt-1.index"]
    rd = T.BundleReader(prefix, verify=True)
    for key in rd.keys():  # every tensor passes its checksum
        rd.get(key)
    assert rd.get("save_counter" + SUF) == 1 and rd.get("save_counter" + SUF).dtype == np.int64
    w, info = T.load_hmr_weights(d)
    assert "object graph" in info["resolved_by"]
    _assert_weights(w, weights)
    np.testing.assert_array_equal(w["inital_theta"], theta0)
    np.testing.assert_array_equal(w["mean_var"].reshape(-1), mean)
    c, cinfo = T.load_critic_weights(d)
    assert "object graph" in cinfo["resolved_by"]
    for key, _off, _shape in critic_spec.flat_layout():
        np.testing.assert_array_equal(c[key], weights[key])


def test_object_graph_has_the_references_roots_and_slot_records(saved):
    _d, prefix, _t, _m, opts = saved
    rd = T.BundleReader(prefix)
    blob = rd.get(T.OBJECT_GRAPH_KEY)
    g = T.ObjectGraph(blob)
    roots = set(g.nodes[0]["children"])
    assert roots == {"generator_optimizer", "discriminator_optimizer", "feature_extractor", "generator3d", "discriminator", "inital_theta",
                     "save_counter", "mean_var"}
    go = g.child(0, "generator_optimizer")
    assert set(g.nodes[go]["children"]) == {"iter", "learning_rate", "beta_1", "beta_2", "decay"}
    assert rd.get(g.variable(g.child(go, "iter"))[1]).dtype == np.int64 and rd.get(g.variable(g.child(go, "decay"))[1]).dtype == np.float32
    fe = g.child(0, "feature_extractor")
    order = T.keras_weighted_layer_order(False)
    assert len(g.nodes[fe]["children"]) == len(order)
    bn = g.child(fe, "layer_with_weights-1")
    assert set(g.nodes[bn]["children"]) == {"gamma", "beta", "moving_mean", "moving_variance"}
    assert g.variable(g.child(bn, "moving_variance")) == ("bn_conv1/moving_variance", "feature_extractor/layer_with_weights-1/moving_variance" + SUF)
    # slot records: (optimizer node, original variable node, "m" | "v", slot node) with the slot key form of tf.train.Checkpoint
    recs = T._graph_slots(blob)
    assert len(recs) == 2 * (len(GEN_SLOT_KEYS) + len(CRITIC_SLOT_KEYS))
    conv1 = g.child(g.child(fe, "layer_with_weights-0"), "kernel")
    mine = [r for r in recs if r[1] == conv1]
    assert sorted(r[2] for r in mine) == ["m", "v"] and all(r[0] == go for r in mine)
    key = g.variable([r for r in mine if r[2] == "m"][0][3])[1]
    assert key == "feature_extractor/layer_with_weights-0/kernel/.OPTIMIZER_SLOT/generator_optimizer/m" + SUF
    np.testing.assert_array_equal(rd.get(key), opts["generator_optimizer"]["slots"]["conv1/kernel"]["m"])
    # numbered breadth-first: every child id is larger than its parent's, the root's children come first
    assert sorted(g.nodes[0]["children"].values()) == list(range(1, 9))


def test_load_training_state_returns_every_slot_and_both_iters(saved, weights):
    d, prefix, _t, mean, opts = saved
    st = T.load_training_state(d)
    assert st["prefix"] == prefix and st["save_counter"] == 1
    np.testing.assert_array_equal(st["mean_var"], mean)
    gen, dis = st["generator_optimizer"], st["discriminator_optimizer"]
    assert gen["iter"] == 2 ** 33 + 5 and dis["iter"] == 7
    assert gen["learning_rate"] == float(np.float32(1e-4)) and dis["learning_rate"] == float(np.float32(5e-4))
    assert gen["beta_1"] == float(np.float32(0.9)) and gen["beta_2"] == float(np.float32(0.999)) and gen["decay"] == 0.0
    for got, want in ((gen, opts["generator_optimizer"]), (dis, opts["discriminator_optimizer"])):
        assert set(got["slots"]) == set(want["slots"])
        for k, mv in want["slots"].items():
            for s in ("m", "v"):
                np.testing.assert_array_equal(got["slots"][k][s].reshape(-1), mv[s].reshape(-1))
    # ... and mapped back to the flat layouts, zeros where a variable has no slots
    tables = T._flat_tables()
    for layout, owner, want in (("encoder", gen, opts["generator_optimizer"]), ("regressor", gen, opts["generator_optimizer"]),
                                ("critic", dis, opts["discriminator_optimizer"])):
        table, total = tables[layout]
        assert owner[layout]["m"].shape == owner[layout]["v"].shape == (total,)
        for k, o, n in table:
            for s in ("m", "v"):
                if k in want["slots"]:
                    np.testing.assert_array_equal(owner[layout][s][o:o + n], want["slots"][k][s].reshape(-1))
                else:
                    assert k in owner["missing"] and not owner[layout][s][o:o + n].any()
    assert tables["encoder"][1] == resnet_spec.ENCODER_PARAM_FLOATS and tables["regressor"][1] == regressor_spec.PARAM_FLOATS


def test_flat_slots_is_the_inverse_of_the_flat_mapping(tmp_path, weights):
    rng = np.random.default_rng(6)
    m, v = rng.normal(size=critic_spec.PARAM_FLOATS).astype(np.float32), rng.random(critic_spec.PARAM_FLOATS).astype(np.float32)
    opts = {"discriminator_optimizer": {"iterations": 3, "learning_rate": 5e-4, "beta_1": 0.9, "beta_2": 0.999, "slots": T.flat_slots("critic", m, v)}}
    T.save_checkpoint(str(tmp_path / "ckpt-2"), weights, optimizers=opts, save_counter=2)
    st = T.load_training_state(str(tmp_path))
    assert "generator_optimizer" not in st and st["discriminator_optimizer"]["missing"] == []
    np.testing.assert_array_equal(st["discriminator_optimizer"]["critic"]["m"], m)
    np.testing.assert_array_equal(st["discriminator_optimizer"]["critic"]["v"], v)
    with pytest.raises(ValueError):
        T.flat_slots("critic", m[:-1], v[:-1])
    with pytest.raises(KeyError):
        T.save_checkpoint(str(tmp_path / "ckpt-3"), weights, optimizers={"generator_optimizer": {"iterations": 1, "slots": {"nope/kernel": {"m": m, "v": v}}}})


def test_weights_only_bundle_has_no_optimiser_state(tmp_path, weights):
    """a weights-only checkpoint from the independent writer loads as weights, and load_training_state says what is missing"""
    tensors, fe, g3 = {}, {}, {}
    for i, layer in enumerate(T.keras_weighted_layer_order(False)):
        node = {}
        for var in (("kernel", "bias") if not layer.startswith("bn") else T._BN_VARS):
            ckey = "feature_extractor/layer_with_weights-%d/%s%s" % (i, var, SUF)
            tensors[ckey] = weights["%s/%s" % (layer, var)]
            node[var] = ("%s/%s" % (layer, var), ckey)
        fe["layer_with_weights-%d" % i] = node
    for i in range(3):
        node = {}
        for var in ("kernel", "bias"):
            ckey = "generator3d/layer_with_weights-%d/%s%s" % (i, var, SUF)
            tensors[ckey] = weights["dense_%d/%s" % (i, var)]
            node[var] = ("dense_%d/%s" % (i, var), ckey)
        g3["layer_with_weights-%d" % i] = node
    tensors[T.OBJECT_GRAPH_KEY] = W.object_graph({"feature_extractor": fe, "generator3d": g3})
    W.write_bundle(str(tmp_path / "ckpt-1"), tensors)
    W.write_checkpoint_state(str(tmp_path), "ckpt-1")
    w, _info = T.load_hmr_weights(str(tmp_path))
    _assert_weights(w, weights)
    with pytest.raises(T.CheckpointError, match="no optimiser state"):
        T.load_training_state(str(tmp_path))
    # the package's writer without optimisers: the same answer
    T.save_checkpoint(str(tmp_path / "ckpt-2"), weights, save_counter=2)
    with pytest.raises(T.CheckpointError, match="no optimiser state"):
        T.load_training_state(str(tmp_path))


def test_two_saves_name_the_newer_and_a_flipped_byte_is_caught(tmp_path):
    small = {"a/kernel" + SUF: np.arange(5000, dtype=np.float32), "b" + SUF: np.array(4, np.int64), "s": b"text"}
    for n in (1, 2):
        T.write_bundle(str(tmp_path / ("ckpt-%d" % n)), small)
        T.write_checkpoint_state(str(tmp_path), "ckpt-%d" % n)
    assert T.latest_checkpoint(str(tmp_path)) == str(tmp_path / "ckpt-2")
    state = open(str(tmp_path / "checkpoint")).read().splitlines()
    assert state == ['model_checkpoint_path: "ckpt-2"', 'all_model_checkpoint_paths: "ckpt-1"', 'all_model_checkpoint_paths: "ckpt-2"']
    rd = T.BundleReader(str(tmp_path / "ckpt-2"))
    np.testing.assert_array_equal(rd.get("a/kernel" + SUF), small["a/kernel" + SUF])
    assert rd.get("s") == b"text" and rd.get("b" + SUF) == 4 and rd.shape("b" + SUF) == ()
    path = str(tmp_path / "ckpt-2.data-00000-of-00001")
    raw = bytearray(open(path, "rb").read())
    raw[1234] ^= 0x10
    open(path, "wb").write(bytes(raw))
    with pytest.raises(T.CheckpointError, match="checksum"):
        T.BundleReader(str(tmp_path / "ckpt-2")).get("a/kernel" + SUF)
    ipath = str(tmp_path / "ckpt-1.index")
    raw = bytearray(open(ipath, "rb").read())
    raw[10] ^= 0x01
    open(ipath, "wb").write(bytes(raw))
    with pytest.raises(T.CheckpointError):
        T.BundleReader(str(tmp_path / "ckpt-1"))


def test_many_keys_span_several_table_blocks(tmp_path):
    """more entries than one 4 KiB block holds, keys with long shared prefixes: restarts, block boundaries and the index block"""
    tensors = {"net/layer_with_weights-%d/kernel/.OPTIMIZER_SLOT/opt/m%s" % (i, SUF): np.full((i % 7 + 1,), i, np.float32) for i in range(600)}
    T.write_bundle(str(tmp_path / "ckpt-1"), tensors)
    assert os.path.getsize(str(tmp_path / "ckpt-1.index")) > 3 * 4096
    rd = T.BundleReader(str(tmp_path / "ckpt-1"))
    assert rd.keys() == sorted(tensors)
    for k, v in tensors.items():
        np.testing.assert_array_equal(rd.get(k), v)
