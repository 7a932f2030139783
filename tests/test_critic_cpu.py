"""CPU-side checks of the critic (no GPU needed): the C ABI, the layer table, the argument checks that come before any device work, the
KCS definition and its closed-form gradient (tests/critic_ref.py), and the checkpoint reader's ``load_critic_weights``."""
import ctypes as C

import numpy as np
import pytest
import torch

import critic_ref as R
import tf_bundle_writer as W
from hpe_amd import _lib, build as hbuild, critic_spec, predictor, synthetic, tf_checkpoint as T

SUF = T.VAR_SUFFIX
P, I, V = C.c_void_p, C.c_int, C.c_void_p


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


def test_abi_symbols_and_argtypes(lib):
    want = {
        "hpe_critic_layer_name": (C.c_char_p, [I]),
        "hpe_critic_layer_shape": (I, [I, C.POINTER(I)]),
        "hpe_load_critic": (I, [P, C.POINTER(_lib.HpeCriticModel)]),
        "hpe_critic": (I, [P, V, I, V, I, V, I, V, V, V]),
        "hpe_critic_backward": (I, [P, V, I, V, I, V, I, V, V, V, V, V, V]),
    }
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype == res and list(fn.argtypes) == args, name
    assert _lib.NUM_CRITIC_DENSE == 9 and C.sizeof(_lib.HpeCriticModel) == 18 * C.sizeof(C.c_void_p)
    hdr = open(hbuild.HERE + "/../include/hpe.h").read()
    assert "#define HPE_NUM_CRITIC_DENSE 9" in hdr
    assert "const float* kernel[HPE_NUM_CRITIC_DENSE];" in hdr and "const float* bias[HPE_NUM_CRITIC_DENSE];" in hdr


def test_layer_table(lib):
    shape = (I * 2)()
    for i, (name, fi, fo, _act) in enumerate(R.LAYERS):
        assert lib.hpe_critic_layer_name(i).decode() == name
        assert lib.hpe_critic_layer_shape(i, shape) == 0 and tuple(shape) == (fi, fo)
    assert lib.hpe_critic_layer_name(9) is None and lib.hpe_critic_layer_name(-1) is None
    assert lib.hpe_critic_layer_shape(9, shape) == 1
    assert tuple((n, i, o) for n, i, o, _ in R.LAYERS) == critic_spec.CRITIC_LAYERS  # the product's one table; its users derive theirs
    assert synthetic.CRITIC_LAYERS is critic_spec.CRITIC_LAYERS and T.CRITIC_SHAPES == {n: (i, o) for n, i, o in critic_spec.CRITIC_LAYERS}
    assert len({(i, o) for _n, i, o, _ in R.LAYERS}) == 9  # what makes assignment by shape unambiguous
    p = synthetic.make_critic_params()
    assert sorted(p) == sorted("critic/%s/%s" % (n, v) for n, _i, _o, _ in R.LAYERS for v in ("kernel", "bias"))
    for n, fi, fo, _ in R.LAYERS:
        k, b = p["critic/%s/kernel" % n], p["critic/%s/bias" % n]
        assert k.shape == (fi, fo) and b.shape == (fo,) and k.dtype == np.float32
        assert np.abs(k).max() <= np.sqrt(6.0 / (fi + fo)) and np.abs(b).min() > 0.0


def test_null_ctx_and_unloaded_ctx(lib):
    """a NULL ctx is HPE_ERR_INVALID (1) before anything else; where a ctx can be created (a gfx950 device is visible), one without a
    critic answers HPE_ERR_STATE (3) -- the pointers are never dereferenced on either path"""
    m = _lib.HpeCriticModel()
    assert lib.hpe_load_critic(None, C.byref(m)) == 1
    assert lib.hpe_critic(None, 8, 14, 8, 10, 8, 1, 8, None, None) == 1
    assert b"null ctx" in lib.hpe_last_error()
    assert lib.hpe_critic_backward(None, 8, 14, 8, 10, 8, 1, None, 8, 8, 8, 8, None) == 1
    cfg = _lib.HpeConfig()
    lib.hpe_config_init(C.byref(cfg))
    h = C.c_void_p()
    rc = lib.hpe_create(C.byref(cfg), C.byref(h))
    assert rc in (0, 4), rc
    if rc == 0:
        try:
            assert lib.hpe_critic(h, 8, 14, 8, 10, 8, 1, 8, None, None) == 3
            assert b"no critic loaded" in lib.hpe_last_error()
            assert lib.hpe_critic_backward(h, 8, 14, 8, 10, 8, 1, None, 8, 8, 8, 8, None) == 3
            assert lib.hpe_load_critic(h, None) == 1
            assert lib.hpe_load_critic(h, C.byref(m)) == 1  # null kernels
        finally:
            lib.hpe_destroy(h)


def test_kcs_gram_equals_the_reference_tensordot():
    """the reference builds an N x 13 x 13 x N tensor and takes its batch diagonal; per row that is the Gram matrix B^T B"""
    g = np.random.default_rng(3)
    for N in (3, 7):
        joints = g.normal(size=(N, 19, 3))
        lit, gram = R.kcs_literal(joints), R.kcs_gram(joints)
        assert lit.shape == gram.shape == (N, 13, 13)
        assert np.abs(lit - gram).max() <= 1e-12
        assert np.allclose(gram, np.transpose(gram, (0, 2, 1)), rtol=0.0, atol=1e-14)
        t = R.CriticTorch({}, torch.float64).kcs(torch.from_numpy(joints)).numpy()
        assert np.abs(t - gram).max() <= 1e-12
    C_ = R.c_matrix()
    assert C_.shape == (14, 13) and (C_.sum(0) == 0).all() and (np.abs(C_).sum(0) == 2).all()


def test_kcs_closed_form_gradient_equals_autograd():
    g = np.random.default_rng(4)
    N = 5
    joints = g.normal(size=(N, 19, 3))
    G = g.normal(size=(N, 13, 13))  # not symmetric: the fold must use G + G^T
    x = torch.from_numpy(joints).requires_grad_(True)
    (R.CriticTorch({}, torch.float64).kcs(x) * torch.from_numpy(G)).sum().backward()
    auto = x.grad.numpy()
    fold = R.kcs_grad_fold(joints, G)
    assert np.abs(auto[:, :14] - fold).max() <= 1e-12 * np.abs(fold).max()
    assert np.abs(auto[:, 14:]).max() == 0.0


# ---------------------------------------------------------------------------------------------------- checkpoint reader
def _bundle(critic, names, order):
    """the discriminator's tensors and its object-graph subtree: slot N of layer_with_weights-N holds layer order[N]; names="keras" gives
    the variables their Keras names, anything else auto-generated ones that say nothing"""
    tensors, disc = {}, {}
    for slot, li in enumerate(order):
        name = R.LAYERS[li][0]
        node = {}
        for var in ("kernel", "bias"):
            ckey = "discriminator/layer_with_weights-%d/%s%s" % (slot, var, SUF)
            tensors[ckey] = critic["critic/%s/%s" % (name, var)]
            full = "%s/%s" % (name if names == "keras" else "dense_%d" % (slot + 11), var)
            node[var] = (full, ckey)
        disc["layer_with_weights-%d" % slot] = node
        disc["layer-%d" % (slot + 4)] = node
    return tensors, disc


def _write(tmp_path, name, hmr_tensors, critic_tensors, tree):
    tensors = dict(hmr_tensors)
    tensors.update(critic_tensors)
    if tree is not None:
        tensors[T.OBJECT_GRAPH_KEY] = W.object_graph(tree)
    else:
        tensors.pop(T.OBJECT_GRAPH_KEY, None)
    W.write_bundle(str(tmp_path / name), tensors)
    return str(tmp_path / name)


@pytest.fixture(scope="module")
def hmr():
    """encoder + regressor tensors and their object-graph tree, built as test_tf_checkpoint does (its stray 10 x 5 discriminator
    kernel is dropped: the bundles below carry a whole discriminator or none)"""
    enc, reg = synthetic.make_encoder_params(seed=1), synthetic.make_regressor_params(seed=2)
    order = T.keras_weighted_layer_order(False)
    tensors, fe, g3 = {}, {}, {}
    for i, layer in enumerate(order):
        node = {}
        for var in (("kernel", "bias") if not layer.startswith("bn") else T._BN_VARS):
            ckey = "feature_extractor/layer_with_weights-%d/%s%s" % (i, var, SUF)
            tensors[ckey] = enc["%s/%s" % (layer, var)]
            node[var] = ("%s/%s" % (layer, var), ckey)
        fe["layer_with_weights-%d" % i] = node
    for i in range(3):
        node = {}
        for var in ("kernel", "bias"):
            ckey = "generator3d/layer_with_weights-%d/%s%s" % (i, var, SUF)
            tensors[ckey] = reg["dense_%d/%s" % (i, var)]
            node[var] = ("dense_%d/%s" % (i + 7, var), ckey)
        g3["layer_with_weights-%d" % i] = node
    tensors["inital_theta" + SUF] = np.random.default_rng(0).normal(size=(1, 85)).astype(np.float32)
    tree = {"feature_extractor": fe, "generator3d": g3, "inital_theta": ("Variable", "inital_theta" + SUF)}
    return tensors, tree


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_load_critic_weights_round_trips(tmp_path, hmr):
    hmr_tensors, tree = hmr
    critic = synthetic.make_critic_params(seed=9)
    # a bundle without a discriminator: the baseline of load_hmr_weights, and a clear error from load_critic_weights
    bare = _write(tmp_path, "ckpt-1", hmr_tensors, {}, dict(tree))
    w0, _ = T.load_hmr_weights(bare)
    with pytest.raises(T.NoCriticError, match="discriminator"):
        T.load_critic_weights(bare)
    with pytest.raises(T.NoCriticError, match="discriminator"):
        T.load_critic_weights(_write(tmp_path, "ckpt-0", hmr_tensors, {}, None))  # ... and without an object graph
    # 1: discriminator under its Keras names, slots scrambled: the names decide
    ct, disc = _bundle(critic, names="keras", order=[4, 0, 8, 2, 6, 1, 7, 3, 5])
    by_name = _write(tmp_path, "ckpt-2", hmr_tensors, ct, dict(tree, discriminator=disc))
    got, info = T.load_critic_weights(by_name)
    assert "object graph" in info["resolved_by"]
    _same(got, critic)
    _same(T.load_hmr_weights(by_name)[0], w0)
    # 2: permuted layer_with_weights-N and names that say nothing (with a graph, and without one): the kernel shapes decide
    ct, disc = _bundle(critic, names="auto", order=[3, 7, 1, 5, 0, 8, 2, 6, 4])
    for name, tr in (("ckpt-3", dict(tree, discriminator=disc)), ("ckpt-4", None)):
        path = _write(tmp_path, name, hmr_tensors, ct, tr)
        got, info = T.load_critic_weights(path)
        assert info["resolved_by"] == "kernel shape"
        _same(got, critic)
        _same(T.load_hmr_weights(path)[0], w0)
    # through a checkpoint directory
    W.write_checkpoint_state(str(tmp_path), "ckpt-2")
    _same(T.load_critic_weights(str(tmp_path))[0], critic)
    # a bias of the wrong length is refused, whichever way the layer was found
    bad = dict(ct)
    bad["discriminator/layer_with_weights-0/bias" + SUF] = np.zeros(7, np.float32)
    with pytest.raises(T.CheckpointError, match="shapes_dense_1"):
        T.load_critic_weights(_write(tmp_path, "ckpt-5", hmr_tensors, bad, None))
    # an incomplete discriminator names what is missing (and is not mistaken for "no discriminator")
    part = {k: v for k, v in ct.items() if "layer_with_weights-1/" not in k}
    incomplete = _write(tmp_path, "ckpt-6", hmr_tensors, part, None)
    with pytest.raises(T.CheckpointError, match="rotation_dense_2") as ei:
        T.load_critic_weights(incomplete)
    assert not isinstance(ei.value, T.NoCriticError)

    # ---- the four places a Predictor takes its critic from (predictor.resolve_critic_params), first match wins
    class Cfg(object):
        critic_params = None

    other = synthetic.make_critic_params(seed=10)
    ck = {"prefix": by_name}
    assert predictor.resolve_critic_params(Cfg()) is None
    assert predictor.resolve_critic_params(Cfg(), weights=w0) is None  # weights.npz without critic/ keys
    assert predictor.resolve_critic_params(Cfg(), weights=w0, checkpoint_info={"prefix": bare}) is None  # no discriminator: passed over
    _same(predictor.resolve_critic_params(Cfg(), weights=w0, checkpoint_info=ck), critic)  # the checkpoint's discriminator
    both = dict(w0, **other)
    assert predictor.resolve_critic_params(Cfg(), weights=both, checkpoint_info=ck) is both  # critic/ keys of weights.npz
    cfg = Cfg()
    cfg.critic_params = critic
    assert predictor.resolve_critic_params(cfg, weights=both, checkpoint_info=ck) is critic  # config.critic_params
    assert predictor.resolve_critic_params(cfg, other, both, ck) is other  # the argument
    # a discriminator that is there but malformed is an error at construction, not a silent "no critic"
    # (by class name: tf_bundle_writer imports the reader as hpe_amd.tf_checkpoint, a second module object of the same file)
    with pytest.raises(ValueError, match="rotation_dense_2") as ei:
        predictor.resolve_critic_params(Cfg(), checkpoint_info={"prefix": incomplete})
    assert type(ei.value).__name__ == "CheckpointError"
