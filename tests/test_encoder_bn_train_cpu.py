"""Encoder training with batch statistics, without a GPU: the restatement of tests/encoder_bn_train_ref.py against float64 autograd of
conv2d + F.batch_norm(training=True) (+ residual) + ReLU on one layer of each class, the vanishing bias gradient, the statistics
layout against the library, and the statistics helpers of resnet_spec."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_bn_train_ref as RB
from hpe_amd import _lib, build as hbuild, resnet_spec, synthetic
from hpe_amd.resnet_spec import CONV_INDEX, CONV_SPECS

# one layer of each class: 1x1, 3x3, strided 1x1, conv1, a projection shortcut (no activation), a 2c layer with residual
CLASSES = {"1x1": ("res5b_branch2a", False, True), "3x3": ("res5b_branch2b", False, True), "1x1s2": ("res5a_branch2a", False, True),
           "conv1": ("conv1", False, True), "shortcut": ("res5a_branch1", False, False), "2c+res": ("res5b_branch2c", True, True)}


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return _lib.load()


def _case(name, B=2, seed=0):
    lname, with_res, relu = CLASSES[name]
    s = CONV_SPECS[CONV_INDEX[lname]]
    g = torch.Generator().manual_seed(seed)
    p = synthetic.make_encoder_params(seed=5)
    p[s.bn_name + "/gamma"] = np.random.default_rng(1).uniform(0.5, 1.5, s.cout).astype(np.float32)
    lt = RB.layer_tensors(p, s)
    hin = 32 if s.kh == 7 else s.hin  # conv1 on a smaller image: the class, not the size
    s = s._replace(hin=hin, hout=hin // s.stride)
    x = torch.randn(B, s.hin, s.hin, s.cin, generator=g, dtype=torch.float64)
    res = torch.randn(B, s.hout, s.hout, s.cout, generator=g, dtype=torch.float64) if with_res else None
    dy = torch.randn(B, s.hout, s.hout, s.cout, generator=g, dtype=torch.float64)
    return s, lt, x, res, dy, relu


def _autograd(s, lt, x, res, dy, relu):
    W, b, gamma, beta = [t.clone().requires_grad_(True) for t in lt[:4]]
    x = x.clone().requires_grad_(True)
    z = F.conv2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), bias=b, stride=s.stride, padding=(s.kh - 1) // 2)
    y = F.batch_norm(z, None, None, gamma, beta, training=True, eps=RB.EPS).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res
    if relu:
        y = torch.relu(y)
    (y * dy).sum().backward()
    return y.detach(), {"dx": x.grad, "dW": W.grad, "db": b.grad, "dgamma": gamma.grad, "dbeta": beta.grad}


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_restatement_matches_autograd(name):
    s, lt, x, res, dy, relu = _case(name)
    y, ref = _autograd(s, lt, x, res, dy, relu)
    got_y, z, mu, var = RB.layer_forward(s, x, lt, res, relu)
    assert torch.allclose(got_y, y, rtol=0, atol=1e-11)
    got = RB.layer_backward(s, x, z, y, dy, lt, gated=relu)
    for k in ("dW", "dgamma", "dbeta") + (("dx",) if s.kh != 7 else ()):
        assert RB.rel(got[k], ref[k]) < 1e-12, (k, RB.rel(got[k], ref[k]))
    # the bias cancels in z - mu: autograd's db is rounding noise, which is why the library writes exactly 0
    assert float(torch.linalg.norm(ref["db"])) < 1e-12 * float(torch.linalg.norm(ref["dbeta"]))
    assert float(got["db"].abs().max()) == 0.0


def test_stat_layout_matches_library(lib):
    assert lib.hpe_encoder_stat_floats() == resnet_spec.ENCODER_STAT_FLOATS == 2 * sum(s.cout for s in CONV_SPECS)
    ch = 0
    for i, (s, off) in enumerate(zip(CONV_SPECS, resnet_spec.ENCODER_STAT_OFFSETS)):
        assert (lib.hpe_encoder_stat_offset(i, 0), lib.hpe_encoder_stat_offset(i, 1)) == off == (ch, resnet_spec.ENCODER_STAT_CHANNELS + ch)
        ch += s.cout
    for idx, which in ((-1, 0), (len(CONV_SPECS), 0), (0, -1), (0, 2)):
        assert lib.hpe_encoder_stat_offset(idx, which) == -1
    assert lib.hpe_encoder_train_ws_floats_batchnorm(0) == 0
    # the raw-output stash is the one thing that grows with the batch: about 11 M floats per image
    grow = lib.hpe_encoder_train_ws_floats_batchnorm(2) - lib.hpe_encoder_train_ws_floats_batchnorm(1)
    assert grow - (lib.hpe_encoder_train_ws_floats(2) - lib.hpe_encoder_train_ws_floats(1)) == sum(s.hout * s.hout * s.cout for s in CONV_SPECS)
    # both reserves' buffers, added up from the lists they allocate from: the values of commit 03ecb51, which added them up by hand
    want = {1: 76083504, 2: 100471088, 3: 124858672, 8: 249155888, 64: 1618530608}
    assert {B: lib.hpe_encoder_train_ws_floats_batchnorm(B) for B in want} == want
    # refusals that need no device
    assert lib.hpe_encoder_train_reserve_batchnorm(None, 1) == 1
    assert lib.hpe_encoder_backward_batchnorm(None, None, 1, None, None, None) == 1
    assert lib.hpe_encoder_update_stats(None, None, 0.9, 1, None) == 1
    # B = 1 on the 7x7 maps is one slice of 49 rows or two; the 56x56 and 112x112 maps are cut into more than one at B = 1 already
    assert lib.hpe_debug_encoder_bn_slices(0, 1) > 1 and lib.hpe_debug_encoder_bn_slices(2, 1) > 1 and 1 <= lib.hpe_debug_encoder_bn_slices(52, 1) <= 2
    assert lib.hpe_debug_encoder_bn_slices(53, 1) == -1 and lib.hpe_debug_encoder_bn_slices(0, 0) == -1


def test_stats_round_trip():
    p = synthetic.make_encoder_params(seed=3)
    stats = resnet_spec.params_to_stats(p)
    assert stats.shape == (resnet_spec.ENCODER_STAT_FLOATS,) and stats.dtype == np.float32
    back = resnet_spec.stats_to_params(stats)
    assert set(back) == {k for k in p if k.endswith(("/moving_mean", "/moving_variance"))}
    for k in back:
        assert np.array_equal(np.asarray(p[k], np.float32), back[k]), k
    om, ov = resnet_spec.ENCODER_STAT_OFFSETS[CONV_INDEX["res3a_branch1"]]
    assert np.array_equal(stats[om:om + 512], p["bn3a_branch1/moving_mean"]) and np.array_equal(stats[ov:ov + 512], p["bn3a_branch1/moving_variance"])
    # with the flat-parameter helpers: a whole encoder, saved and restored
    q = resnet_spec.flat_to_params(resnet_spec.params_to_flat(p), resnet_spec.stats_to_params(torch.from_numpy(stats)))
    assert set(q) == set(p) and all(np.array_equal(np.asarray(p[k], np.float32), q[k]) for k in p)
    with pytest.raises(ValueError):
        resnet_spec.stats_to_params(stats[:-1])


def test_momentum_update():
    g = torch.Generator().manual_seed(1)
    n = resnet_spec.ENCODER_STAT_FLOATS
    stats, batch = torch.rand(n, generator=g, dtype=torch.float64), torch.rand(n, generator=g, dtype=torch.float64)
    plain = RB.momentum_update(stats, batch, 3, 0.9, False)
    assert torch.allclose(plain, 0.9 * stats + 0.1 * batch, rtol=0, atol=1e-15)
    unb = RB.momentum_update(stats, batch, 3, 0.9, True)
    ch = resnet_spec.ENCODER_STAT_CHANNELS
    assert torch.equal(unb[:ch], plain[:ch])  # the means do not care
    om, ov = resnet_spec.ENCODER_STAT_OFFSETS[52]  # a 7x7 map at B = 3: M = 147
    assert torch.allclose(unb[ov:ov + 4], 0.9 * stats[ov:ov + 4] + 0.1 * batch[ov:ov + 4] * 147.0 / 146.0, rtol=0, atol=1e-15)
